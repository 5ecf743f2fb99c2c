"""Shared by tests/test_host_bn.py and tests/test_hip_bn.py: the host Philox and the dropout keep rule of the BatchNorm +
LeakyReLU + dropout kernels (csrc/bn_act.hip, csrc/bn_fwd_strip.h), their float64 reference and its float32 restatement, the
error measures, the seeded inputs and the case table.  numpy and plain torch on the CPU; no GPU code."""
import functools
import math

import numpy as np
import torch

M32 = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------
# Philox4x32-10 and the keep rule
# ------------------------------------------------------------------------------------------------
def philox4x32_10(counter, key):
    """Philox4x32 with 10 rounds (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11):
    `counter` = four and `key` = two arrays (or ints) of 32-bit words, broadcast against one another; returns the four output
    words as uint64 arrays holding 32-bit values.  A round multiplies counter words 0 and 2 by the two constants, and the new
    words are (hi(p1) ^ c1 ^ k0, lo(p1), hi(p0) ^ c3 ^ k1, lo(p0)); the key is bumped by the Weyl constants between rounds."""
    c0, c1, c2, c3 = (np.asarray(x, dtype=np.uint64) & M32 for x in counter)
    k0, k1 = (np.asarray(x, dtype=np.uint64) & M32 for x in key)
    mul0, mul1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    weyl0, weyl1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = mul0 * c0, mul1 * c2                        # < 2^64: both factors are below 2^32
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & M32, (p0 >> s32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + weyl0) & M32, (k1 + weyl1) & M32
    return c0, c1, c2, c3


def drop_threshold(p):
    """thr = trunc(float32(p) * 65536) clamped to [0, 65535]; the product is formed in float32 as the kernels do."""
    t = float(np.float32(p) * np.float32(65536.0))
    return 0 if t <= 0 else (65535 if t >= 65535 else int(t))


def keep_rate(p):
    """The probability that an element is kept: 1 - thr / 65536 (0.4000092 at p = 0.6), not 1 - p."""
    return 1.0 - drop_threshold(p) / 65536.0


def keep_mask(seed, step, stream, B, N, p):
    """The dropout keep decision of element (row, col) of a [B, N] activation, bool [B, N] -- THE CONTRACT every BatchNorm
    kernel (dword and float4, forward and backward) implements, a pure function of (seed, step, stream, row, col):

        rk      = (row & 127) | ((row >> 8) << 7)
        counter = (rk, col >> 2, stream, low 32 bits of step)
        key     = (low 32 bits of seed, high 32 bits of seed XOR high 32 bits of step)
        word    = philox4x32_10(counter, key)[col & 3]
        half    = (row >> 7) & 1            (0: bits 0..15 of the word, 1: bits 16..31)
        keep    = half-word >= thr,  thr = trunc(float32(p) * 65536) clamped to [0, 65535]

    so one Philox call serves the four columns of a quad in the two rows r and r + 128.  The keep probability is
    1 - thr / 65536 while the survivors are scaled by 1 / (1 - p).  seed and step are unsigned 64-bit values."""
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    row = np.arange(B, dtype=np.uint64)[:, None]
    col = np.arange(N, dtype=np.uint64)[None, :]
    rk = (row & np.uint64(127)) | ((row >> np.uint64(8)) << np.uint64(7))
    quad = col >> np.uint64(2)
    # one call per (rk, quad): the pairs of rows 128 apart share it
    rk_u, rk_inv = np.unique(rk[:, 0], return_inverse=True)
    q_u, q_inv = np.unique(quad[0], return_inverse=True)
    words = philox4x32_10((rk_u[:, None], q_u[None, :], np.uint64(stream & 0xFFFFFFFF), np.uint64(step & 0xFFFFFFFF)),
                          (np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) ^ (step >> 32))))
    words = np.stack([np.broadcast_to(w, (len(rk_u), len(q_u))) for w in words])             # [4, rk, quad]
    w = words[(col & np.uint64(3)).astype(np.int64), rk_inv[:, None], q_inv[None, :]]
    half = (w >> (np.uint64(16) * ((row >> np.uint64(7)) & np.uint64(1)))) & np.uint64(0xFFFF)
    return torch.from_numpy(half >= np.uint64(drop_threshold(p)))


# ------------------------------------------------------------------------------------------------
# panel layout (include/jamie_hip.h: JAMIE_PANEL)
# ------------------------------------------------------------------------------------------------
def to_panels(t, P, fill=0.0):
    """[S, B, N] row-major -> the same values in panels of P columns: flat [S, ceil(N / P) * P * B]; element (row, col) of a
    slab at ((col // P) * B + row) * P + col % P; the padding columns of a ragged last panel hold `fill`."""
    S, B, N = t.shape
    npad = (N + P - 1) // P * P
    p = torch.full((S, B, npad), fill, dtype=t.dtype, device=t.device)
    p[:, :, :N] = t
    return p.reshape(S, B, npad // P, P).permute(0, 2, 1, 3).contiguous().reshape(S, -1)


def from_panels(flat, B, N, P):
    """The inverse of to_panels: [S, ceil(N / P) * P * B] -> ([S, B, N], the padding columns [S, B, npad - N])."""
    S = flat.shape[0]
    npad = (N + P - 1) // P * P
    full = flat.reshape(S, npad // P, B, P).permute(0, 2, 1, 3).reshape(S, B, npad)
    return full[:, :, :N], full[:, :, N:]


# ------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------
def given(x):
    """A hyper-parameter as the kernel receives it: rounded to float32 once, widened."""
    return float(np.float32(x))


def colsum(x):
    """Column sums of [B, N] by a fixed pairwise tree of elementwise additions (rows 2i and 2i + 1, an odd last row carried):
    every addition is one IEEE operation, so the float32 restatement gives the same bits on any machine, whatever order a
    library's reduction takes there."""
    while x.shape[0] > 1:
        n = x.shape[0] // 2 * 2
        x = torch.cat([x[0:n:2] + x[1:n:2], x[n:]])
    return x[0]


def bn_ref(hs, gamma, beta, keep, p, das, rm0, rv0, acc0=None, momentum=0.1, eps=1e-5, slope=0.01, dtype=torch.float64):
    """BatchNorm1d (training statistics) + LeakyReLU + dropout, forward and backward, in `dtype`: float64 is the reference,
    float32 the restatement that fixes the GPU bounds.  hs, das: [S, B, N] split-K slabs of the pre-activation and of the
    upstream gradient (added in slab order); keep: bool [B, N] or None (p == 0); rm0, rv0: running statistics before the
    launch; acc0: None or the (dgamma, dbeta, dbias) already in the buffers of an accumulating launch.  The hyper-parameters
    are read as the kernel is given them (float32).  Returns a dict of `dtype` tensors."""
    p, momentum, eps, slope = given(p), given(momentum), given(eps), given(slope)
    c = lambda t: t.to(dtype)
    h = c(hs[0]).clone()
    for s in range(1, hs.shape[0]):
        h = h + c(hs[s])
    B = h.shape[0]
    gamma, beta = c(gamma), c(beta)
    mean = colsum(h) / B                                   # two-pass: mean, then the biased variance about it
    d = h - mean
    var = colsum(d * d) / B
    invstd = 1.0 / torch.sqrt(var + eps)
    unb = var * (B / (B - 1)) if B > 1 else var
    rm = (1.0 - momentum) * c(rm0) + momentum * mean
    rv = (1.0 - momentum) * c(rv0) + momentum * unb
    xn = d * invstd
    y = xn * gamma + beta
    pos = y > 0                                           # strict: y == 0 takes the slope
    out = torch.where(pos, y, slope * y)
    scale = 1.0 / (1.0 - p)
    if p > 0:
        out = torch.where(keep, out * scale, torch.zeros_like(out))
    da = c(das[0]).clone()
    for s in range(1, das.shape[0]):
        da = da + c(das[s])
    dd = torch.where(keep, da * scale, torch.zeros_like(da)) if p > 0 else da
    dd = torch.where(pos, dd, dd * slope)
    dbeta = colsum(dd)
    dgamma = colsum(dd * xn)
    dh = gamma * invstd * (dd - dbeta / B - xn * (dgamma / B))
    dbias = colsum(dh)
    r = dict(h=h, out=out, y=y, save_mean=mean, save_invstd=invstd, running_mean=rm, running_var=rv, dh=dh,
             dgamma=dgamma, dbeta=dbeta, dbias=dbias, da=da,
             abs_dd=dd.abs().sum(0), abs_ddxn=(dd * xn).abs().sum(0), abs_dh=dh.abs().sum(0))
    if acc0 is not None:
        r['dgamma'], r['dbeta'], r['dbias'] = c(acc0[0]) + dgamma, c(acc0[1]) + dbeta, c(acc0[2]) + dbias
    return r


# ------------------------------------------------------------------------------------------------
# error measures: one number per quantity
# ------------------------------------------------------------------------------------------------
def _d(t):
    return t.detach().cpu().double()


def e_abs1(x, ref):
    """e_y: max |x - ref| / (1 + |ref|)."""
    x, ref = _d(x), _d(ref)
    return float(((x - ref).abs() / (1 + ref.abs())).max())


def e_rel(x, ref):
    """e_stat: max |x - ref| / |ref|."""
    x, ref = _d(x), _d(ref)
    return float(((x - ref).abs() / ref.abs()).max())


def e_col(x, ref, den, cols=None, slack=None):
    """max over the columns `cols` (bool [N]; default all) of |x - ref| / den, den [N] per column.  Where den is 0 the
    difference must be 0 (error 0) or the error is inf.  `slack`: an absolute allowance taken off |x - ref| first (the
    rounding of a bf16 output)."""
    x, ref, den = _d(x), _d(ref), _d(den)
    diff = (x - ref).abs()
    if slack is not None:
        diff = (diff - _d(slack)).clamp(min=0)
    e = torch.where(diff == 0, torch.zeros_like(diff), diff / den.expand_as(diff))       # (x / 0 = inf for x > 0)
    if cols is not None:
        e = e[..., cols]
    return float(e.max()) if e.numel() else 0.0


def fwd_errors(got, ref):
    """got: dict with any of h, out, save_mean, save_invstd, running_mean, running_var -> {name: error}."""
    hmax = ref['h'].abs().max(0).values
    e = {}
    for k in ('h', 'out'):
        if k in got:
            e[k] = e_abs1(got[k], ref[k])
    for k in ('save_mean', 'running_mean'):
        if k in got:
            e[k] = e_col(got[k], ref[k], hmax)
    for k in ('save_invstd', 'running_var'):
        if k in got:
            e[k] = e_rel(got[k], ref[k])
    return e


def bwd_errors(got, ref, cols):
    """got: dict with any of dh, dgamma, dbeta, dbias; `cols`: the columns that take part (kink_columns left out)."""
    den = dict(dh=ref['dh'].abs().max(0).values, dgamma=ref['abs_ddxn'], dbeta=ref['abs_dd'], dbias=ref['abs_dh'])
    return {k: e_col(got[k], ref[k], den[k], cols) for k in ('dh', 'dgamma', 'dbeta', 'dbias') if k in got}


# The float32 restatement (bn_ref with dtype float32) against the float64 reference, maximum over the whole case table and
# the accumulating variants, rounded up to two digits; measured by tests/test_host_bn.py, which also asserts that they are
# the measurement (>= 0.8 of the constant), not a cap.  The GPU bounds are 4 x these, the margin of the optimiser tests:
# the device adds 128 or 16 row phases, then waves, in another order than the restatement's pairwise tree (colsum).
F32_E = dict(y=3.7e-6, mean=1.1e-7, stat=1.7e-7, dh=9.0e-7, dg=4.9e-7, db=2.1e-7, dl=4.2e-7)
KIND = dict(h='y', out='y', save_mean='mean', running_mean='mean', save_invstd='stat', running_var='stat',
            dh='dh', dgamma='dg', dbeta='db', dbias='dl')
BOUND = {k: 4 * v for k, v in F32_E.items()}
# A column is left out of the backward comparisons of a case when a kept element's pre-activation lies within twice the
# forward bound of the LeakyReLU kink: there float32 and float64 may disagree on the sign, one dd changes by 1 / slope and
# the whole column moves.  (The forward comparison leaves nothing out: `out` is continuous there.)
KINK = 2 * BOUND['y']
MAX_KINK_SHARE = 0.05
BF16_HALF_ULP = 2.0 ** -8          # round-to-nearest to 8 significant bits: at most half an ulp = 2^-8 of the value


def kink_columns(ref, keep):
    """bool [N]: a kept element of the column has |y_ref| <= KINK."""
    near = ref['y'].abs() <= KINK
    if keep is not None:
        near = near & keep
    return near.any(0)


def check(errors, label=''):
    """Print every figure, then assert each against its bound."""
    print(label, ' '.join(f'{k} {v:.2e}' for k, v in errors.items()))
    bad = {k: (v, BOUND[KIND[k]]) for k, v in errors.items() if not v <= BOUND[KIND[k]]}
    assert not bad, (label, bad)


# ------------------------------------------------------------------------------------------------
# inputs and the case table
# ------------------------------------------------------------------------------------------------
def make_problem(B, N, nslab, seed):
    """Per column: scale 2^k (k in -6..6), offset within +-4 standard deviations, gamma in +-[0.5, 1.5], beta ~ N(0, 1),
    random running statistics of the column's size, upstream gradient ~ N(0, 1).  With N >= 16 column N - 3 (the last quad) is
    constant: every slab holds a dyadic value, beta = +-0.5, so variance 0, invstd 1 / sqrt(eps) and y = beta exactly."""
    g = torch.Generator().manual_seed(seed)
    scale = 2.0 ** torch.randint(-6, 7, (N,), generator=g).float()
    offset = (torch.rand(N, generator=g) * 8 - 4) * scale
    hs = torch.randn(nslab, B, N, generator=g) * (scale / math.sqrt(nslab)) + offset / nslab
    das = torch.randn(nslab, B, N, generator=g) / math.sqrt(nslab)
    sign = torch.where(torch.rand(N, generator=g) < 0.5, -1.0, 1.0)
    gamma = (0.5 + torch.rand(N, generator=g)) * sign
    beta = torch.randn(N, generator=g)
    rm0 = offset + scale * torch.randn(N, generator=g)
    rv0 = scale * scale * (0.5 + 1.5 * torch.rand(N, generator=g))
    acc0 = tuple(torch.randn(N, generator=g) for _ in range(3))
    const = None
    if N >= 16:
        const = N - 3
        for s in range(nslab):
            hs[s, :, const] = 0.25 * (s + 1)
        beta[const] = 0.5 if seed % 2 else -0.5
        rm0[const], rv0[const] = 0.375, 1.75
    return dict(B=B, N=N, nslab=nslab, hs=hs, das=das, gamma=gamma, beta=beta, rm0=rm0, rv0=rv0, acc0=acc0, const=const)


# seed, step of the rng state (both with high words in use), and the per-problem streams
SEED, STEP = 0x0123456789ABCDEF, 5
DEFAULT_HYPER = dict(momentum=0.1, eps=1e-5, slope=0.01)
# id -> problems [(B, N, nslab, data seed)], p, outputs ('f' fp32, 'b' bf16, 't' transposed bf16), and options:
#   mask 'rng' | 'bytes' (explicit byte mask), panel, offset (floats between the allocation and h / da), hyper
CASES = {
    'c01_quad': dict(probs=[(8, 4, 1, 101)], p=0.0, outs='f'),
    'c02_b136': dict(probs=[(136, 72, 4, 102)], p=0.6, outs='fbt'),
    'c03_production': dict(probs=[(512, 264, 3, 103)], p=0.6, outs='bt'),
    'c04_cq8': dict(probs=[(136, 4116, 2, 104)], p=0.6, outs='fb'),
    'c05_cq8_group': dict(probs=[(136, 2060, 1, 105), (64, 2056, 2, 1050)], p=0.25, outs='b'),
    'c06_r8': dict(probs=[(1024, 136, 3, 106)], p=0.25, outs='fbt'),
    'c07_r8_group': dict(probs=[(1000, 24, 2, 107), (64, 40, 1, 1070), (520, 20, 5, 10700)], p=0.6, outs='fb'),
    'c08_dword': dict(probs=[(200, 33, 4, 108)], p=0.6, outs='fbt'),
    'c09_uncached': dict(probs=[(1032, 24, 2, 109)], p=0.25, outs='f'),
    'c10_misaligned': dict(probs=[(512, 264, 3, 103)], p=0.6, outs='f', offset=1),
    'c11_panel_r4': dict(probs=[(256, 72, 2, 111)], p=0.6, outs='bt', panel=True),
    'c11_panel_r8': dict(probs=[(1024, 136, 2, 1110)], p=0.6, outs='bt', panel=True),
    'c12_bytes': dict(probs=[(136, 72, 4, 102)], p=0.6, outs='f', mask='bytes'),
    'c13_hyper': dict(probs=[(136, 72, 4, 102)], p=0.25, outs='f', hyper=dict(momentum=0.3, eps=1e-3, slope=0.2)),
}
ACCUMULATE_CASES = ('c02_b136', 'c06_r8', 'c08_dword')
READOUT_CASES = ('c02_b136', 'c04_cq8', 'c06_r8', 'c08_dword', 'c09_uncached')
RIDER_CASES = ('c03_production', 'c08_dword')


def stream_of(i):
    return 3 + 2 * i


@functools.lru_cache(maxsize=None)
def case_data(cid):
    """The case's problems with their keep masks and float64 references (computed once, shared, never written to):
    list of dicts make_problem + keep, ref, ref_acc (accumulating launch), cols (columns of the backward comparisons)."""
    case = CASES[cid]
    hyper = case.get('hyper', DEFAULT_HYPER)
    out = []
    for i, (B, N, nslab, seed) in enumerate(case['probs']):
        d = make_problem(B, N, nslab, seed)
        p = case['p']
        if p == 0:
            d['keep'] = None
        elif case.get('mask') == 'bytes':
            d['keep'] = torch.rand(B, N, generator=torch.Generator().manual_seed(seed + 1)) >= p
        else:
            d['keep'] = keep_mask(SEED, STEP, stream_of(i), B, N, p)
        d['ref'] = bn_ref(d['hs'], d['gamma'], d['beta'], d['keep'], p, d['das'], d['rm0'], d['rv0'], **hyper)
        d['ref_acc'] = dict(d['ref'])
        for k, a in zip(('dgamma', 'dbeta', 'dbias'), d['acc0']):
            d['ref_acc'][k] = d['ref'][k] + a.double()
        d['kink'] = kink_columns(d['ref'], d['keep'])
        d['cols'] = ~d['kink']
        d['p'], d['hyper'], d['stream'] = p, hyper, stream_of(i)
        out.append(d)
    return out


# One constant column (column 1) with beta = 0: xn = 0 and y = 0 EXACTLY, in float32 as in float64, so the strict `y > 0` is
# decided by the rule alone and not by rounding -- the element takes the slope.  One problem per backward kernel; the column
# takes part in the comparisons although it sits on the kink.
ZERO_COLUMN = 1
ZERO_CASES = {'z_float4_r4': (136, 20, 201), 'z_float4_r8': (520, 20, 202), 'z_dword': (40, 17, 203), 'z_uncached': (1032, 8, 204)}


@functools.lru_cache(maxsize=None)
def zero_case_data(zid):
    B, N, seed = ZERO_CASES[zid]
    d = make_problem(B, N, 1, seed)
    d['hs'][0, :, ZERO_COLUMN] = -1.5
    d['beta'][ZERO_COLUMN] = 0.0
    d['rm0'][ZERO_COLUMN], d['rv0'][ZERO_COLUMN] = 0.375, 1.75          # (of the column's size, like every other column's)
    d['p'], d['hyper'], d['stream'] = 0.25, DEFAULT_HYPER, 9
    d['keep'] = keep_mask(SEED, STEP, d['stream'], B, N, d['p'])
    d['ref'] = bn_ref(d['hs'], d['gamma'], d['beta'], d['keep'], d['p'], d['das'], d['rm0'], d['rv0'])
    d['ref_acc'] = None
    d['kink'] = kink_columns(d['ref'], d['keep'])
    d['cols'] = ~d['kink']
    d['cols'][ZERO_COLUMN] = True
    return d


def restatement_errors(d, accumulate=False):
    """The float32 restatement of one problem against its float64 reference: {quantity: error}."""
    r32 = bn_ref(d['hs'], d['gamma'], d['beta'], d['keep'], d['p'], d['das'], d['rm0'], d['rv0'],
                 acc0=d['acc0'] if accumulate else None, dtype=torch.float32, **d['hyper'])
    ref = d['ref_acc'] if accumulate else d['ref']
    e = fwd_errors(r32, ref)
    e.update(bwd_errors(r32, ref, d['cols']))
    return e

"""The BatchNorm + LeakyReLU + dropout kernels (csrc/bn_act.hip, csrc/bn_fwd_strip.h) in the forms the engine launches, against
the float64 reference and the host Philox of tests/bn_util.py: every instance the launcher can pick (dword cached / uncached,
float4 with 4 or 8 rows per thread, 16- and 32-column strips), grouped launches of unequal problems, bf16 row-major and
transposed outputs, panel inputs, split-K slabs with NaN between them, and the dropout mask bit for bit.  The bounds are
4 x the float32 restatement's errors (tests/test_host_bn.py); every figure is printed before it is asserted.
Run on the MI355X box:  pytest -m gpu tests/test_hip_bn.py"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_util as bu  # noqa: E402

pytestmark = pytest.mark.gpu

TAIL = 64          # over-allocation of every output, NaN before the launch and after
NAN = float('nan')


@pytest.fixture(scope='module')
def nv():
    from jamie_amd import _native
    _native.require_gpu()
    return _native


def dev(t):
    return t.to('cuda').contiguous()


def nanbuf(n, dtype=torch.float32):
    return torch.full((n,), NAN, dtype=dtype, device='cuda')


def with_tail(v):
    return torch.cat([dev(v), nanbuf(8)])


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a.contiguous()), bits(b.contiguous()))


def rng_state(seed=bu.SEED, step=bu.STEP):
    as_i64 = lambda x: x - (1 << 64) if x >= (1 << 63) else x
    return torch.tensor([as_i64(seed), as_i64(step), 0, 0], dtype=torch.int64, device='cuda')


def pw(nv):
    return int(nv.load().jamie_panel_width())


def slab_buffer(slabs, panel, offset, P):
    """[S, B, N] host slabs -> (device view that starts `offset` floats into its allocation, slab stride, floats of one slab).
    The slabs lie a stride apart that is larger than one slab (a multiple of 4 floats where N is one); the gaps, the padding
    columns of a ragged last panel and a tail are NaN, so a load past a slab's end poisons the result."""
    S, B, N = slabs.shape
    flat = bu.to_panels(slabs, P, NAN) if panel else slabs.reshape(S, -1)
    one = flat.shape[1]
    stride = one + (8 if N % 4 == 0 else 5)
    buf = nanbuf(offset + (S - 1) * stride + one + TAIL)
    view = buf[offset:]
    for s in range(S):
        view[s * stride:s * stride + one] = dev(flat[s])
    return view, stride, one


class Prob:
    """The device buffers of one problem of a launch."""

    def __init__(self, nv, d, outs, panel=False, offset=0, readout=False, stream=None, bytes_mask=False):
        self.nv, self.d, self.panel, self.P, self.offset = nv, d, panel, pw(nv), offset
        B, N = d['B'], d['N']
        self.h, self.stride, self.one = slab_buffer(d['hs'], panel, offset, self.P)
        self.h_pre = self.h.clone()
        self.gamma = dev(torch.zeros(N) if readout else d['gamma'])
        self.beta = dev(torch.ones(N) if readout else d['beta'])
        self.rm, self.rv, self.sm, self.si = with_tail(d['rm0']), with_tail(d['rv0']), nanbuf(N + 8), nanbuf(N + 8)
        self.out = nanbuf(B * N + TAIL) if 'f' in outs else None
        self.out_bf = nanbuf(B * N + TAIL, torch.bfloat16) if 'b' in outs else None
        self.outT_bf = nanbuf(B * N + TAIL, torch.bfloat16) if 't' in outs else None
        self.mask = dev(d['keep'].to(torch.uint8)) if bytes_mask else None
        self.stream = d['stream'] if stream is None else stream

    def fwd_problem(self):
        nv, d, pr = self.nv, self.d, self.nv.BnFwdProblem()
        pr.h, pr.nslab, pr.slab_stride = nv.ptr(self.h), d['nslab'], self.stride
        pr.gamma, pr.beta = nv.ptr(self.gamma), nv.ptr(self.beta)
        pr.running_mean, pr.running_var, pr.save_mean, pr.save_invstd = nv.ptr(self.rm), nv.ptr(self.rv), nv.ptr(self.sm), nv.ptr(self.si)
        pr.out, pr.mask, pr.B, pr.N, pr.rng_stream = nv.ptr(self.out), nv.ptr(self.mask), d['B'], d['N'], self.stream
        pr.out_bf16, pr.outT_bf16, pr.panel = nv.ptr(self.out_bf), nv.ptr(self.outT_bf), int(self.panel)
        return pr

    def prep_bwd(self, outs, accumulate=False, dbias=True, offset=None):
        d = self.d
        offset = self.offset if offset is None else offset
        B, N = d['B'], d['N']
        self.da, self.da_stride, self.da_one = slab_buffer(d['das'], self.panel, offset, self.P)
        self.da_pre = self.da.clone()
        self.accumulate, self.skip = accumulate, 'f' not in outs
        acc = [with_tail(a) for a in d['acc0']] if accumulate else [nanbuf(N + 8) for _ in range(3)]
        self.dg, self.db, self.dl = acc[0], acc[1], (acc[2] if dbias else None)
        self.dh_bf = nanbuf(B * N + TAIL, torch.bfloat16) if 'b' in outs else None
        self.dhT_bf = nanbuf(B * N + TAIL, torch.bfloat16) if 't' in outs else None

    def bwd_problem(self):
        nv, d, pb = self.nv, self.d, self.nv.BnBwdProblem()
        pb.da, pb.nslab, pb.slab_stride = nv.ptr(self.da), d['nslab'], self.da_stride
        pb.h, pb.gamma, pb.beta, pb.save_mean, pb.save_invstd = nv.ptr(self.h), nv.ptr(self.gamma), nv.ptr(self.beta), nv.ptr(self.sm), nv.ptr(self.si)
        pb.dgamma, pb.dbeta, pb.dbias_lin, pb.mask = nv.ptr(self.dg), nv.ptr(self.db), nv.ptr(self.dl), nv.ptr(self.mask)
        pb.B, pb.N, pb.rng_stream, pb.accumulate = d['B'], d['N'], self.stream, int(self.accumulate)
        pb.dh_bf16, pb.dhT_bf16, pb.skip_f32, pb.panel = nv.ptr(self.dh_bf), nv.ptr(self.dhT_bf), int(self.skip), int(self.panel)
        return pb


def make_probs(nv, cid, outs):
    case = bu.CASES[cid]
    return [Prob(nv, d, outs, panel=case.get('panel', False), offset=case.get('offset', 0),
                 bytes_mask=case.get('mask') == 'bytes') for d in bu.case_data(cid)]


def launch_fwd(nv, probs, state=None):
    d = probs[0].d                                   # (p and the hyper-parameters travel with the data)
    state = rng_state() if state is None else state
    nv.bn_act_fwd([P.fwd_problem() for P in probs], d['p'], None if probs[0].mask is not None or d['p'] == 0 else state, **d['hyper'])
    torch.cuda.synchronize()


def launch_bwd(nv, probs, colsums=None):
    d = probs[0].d
    nv.bn_act_bwd([P.bwd_problem() for P in probs], d['p'], None if probs[0].mask is not None or d['p'] == 0 else rng_state(),
                  slope=d['hyper']['slope'], colsums=colsums)
    torch.cuda.synchronize()


def tail_is_nan(t, n):
    return bool(torch.isnan(t[n:].float()).all())


def check_fwd(P, label):
    """Everything a forward launch wrote against the reference; everything it should not have written still as it was."""
    d, ref = P.d, P.d['ref']
    B, N, S = d['B'], d['N'], d['nslab']
    # the slabs after the first, the NaN between and behind them: untouched
    assert same_bits(P.h[P.one:], P.h_pre[P.one:]), label
    if S == 1:
        assert same_bits(P.h, P.h_pre), label
    if P.panel:
        h0, pad = bu.from_panels(P.h[:P.one][None], B, N, P.P)
        assert bool(torch.isnan(pad).all()), label             # padding columns of the ragged last panel
        h0 = h0[0]
    else:
        h0 = P.h[:P.one].reshape(B, N)
    got = dict(h=h0, save_mean=P.sm[:N], save_invstd=P.si[:N], running_mean=P.rm[:N], running_var=P.rv[:N])
    for t in (P.sm, P.si, P.rm, P.rv):
        assert tail_is_nan(t, N), label
    if P.out is not None:
        got['out'] = P.out[:B * N].reshape(B, N)
        assert tail_is_nan(P.out, B * N), label
    bu.check(bu.fwd_errors(got, ref), label + ' fwd')
    for name, t, tr in (('out_bf16', P.out_bf, False), ('outT_bf16', P.outT_bf, True)):
        if t is None:
            continue
        assert tail_is_nan(t, B * N), (label, name)
        v = t[:B * N].reshape(N, B).t() if tr else t[:B * N].reshape(B, N)
        got[name] = v
        if P.out is not None:
            assert same_bits(v, got['out'].to(torch.bfloat16)), (label, name)
        else:       # |x - ref| <= 2^-8 |x'| + |x' - ref|, x' the fp32 value that was rounded: the bound plus half a bf16 ulp
            r = ref['out']
            lim = bu.BOUND['y'] * (1 + r.abs())
            over = (v.float().cpu().double() - r).abs() - bu.BF16_HALF_ULP * (r.abs() + lim)
            e = float((over.clamp(min=0) / (1 + r.abs())).max())
            print(label, name, f'beyond bf16 rounding {e:.2e}')
            assert e <= bu.BOUND['y'], (label, name, e)
    return got


def check_bwd(P, label, full=None):
    """The same for a backward launch.  `full`: the results of the launch that also wrote fp32 (bit-identical bf16 expected)."""
    d = P.d
    ref = d['ref_acc'] if P.accumulate else d['ref']
    B, N = d['B'], d['N']
    got = dict(dgamma=P.dg[:N], dbeta=P.db[:N])
    if P.dl is not None:
        got['dbias'] = P.dl[:N]
    for t in (P.dg, P.db, P.dl):
        assert t is None or tail_is_nan(t, N), label
    if P.skip:
        assert same_bits(P.da, P.da_pre), label                 # the fp32 gradient buffer: not written at all
    else:
        assert same_bits(P.da[P.da_one:], P.da_pre[P.da_one:]), label
        got['dh'] = P.da[:B * N].reshape(B, N)
    bu.check(bu.bwd_errors(got, ref, d['cols']), label + (' bwd acc' if P.accumulate else ' bwd'))
    colmax = ref['dh'].abs().max(0).values
    for name, t, tr in (('dh_bf16', P.dh_bf, False), ('dhT_bf16', P.dhT_bf, True)):
        if t is None:
            continue
        assert tail_is_nan(t, B * N), (label, name)
        v = t[:B * N].reshape(N, B).t() if tr else t[:B * N].reshape(B, N)
        got[name] = v
        if not P.skip:
            assert same_bits(v, got['dh'].to(torch.bfloat16)), (label, name)
        else:
            # |x - ref| <= 2^-8 |x'| + |x' - ref| with x' the fp32 value that was rounded: the dh bound plus half a bf16 ulp
            e = bu.e_col(v.float(), ref['dh'], colmax, d['cols'], slack=bu.BF16_HALF_ULP * (ref['dh'].abs() + bu.BOUND['dh'] * colmax))
            print(label, name, f'beyond bf16 rounding {e:.2e}')
            assert e <= bu.BOUND['dh'], (label, name, e)
            if full is not None:
                assert same_bits(v, full[name]), (label, name)
    return got


# ------------------------------------------------------------------------------------------------
# every case against float64
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cid', list(bu.CASES))
def test_case_against_fp64(nv, cid):
    """Forward, then backward, of every row of the case table.  A case whose outputs are bf16 only (out = NULL, skip_f32: the
    engine's form) runs twice: once with the fp32 outputs beside the bf16 ones, held to the bounds, once as the engine launches
    it, whose bf16 tensors must then be the same bits.  (A panel backward launch cannot write fp32 dh: its bf16 dh is held to
    the dh bound plus half a bf16 ulp.)"""
    case = bu.CASES[cid]
    outs = case['outs']
    panel = case.get('panel', False)
    full_outs = outs if 'f' in outs else 'f' + outs
    probs = make_probs(nv, cid, full_outs)
    launch_fwd(nv, probs)
    f_full = [check_fwd(P, f'{cid}[{i}]') for i, P in enumerate(probs)]
    b_full = [None] * len(probs)
    if not panel:
        for P in probs:
            P.prep_bwd(full_outs)
        launch_bwd(nv, probs)
        b_full = [check_bwd(P, f'{cid}[{i}]') for i, P in enumerate(probs)]
    if 'f' in outs:
        return
    prod = make_probs(nv, cid, outs)
    launch_fwd(nv, prod)
    for i, P in enumerate(prod):
        g = check_fwd(P, f'{cid}[{i}] bf16 only')
        for name in ('out_bf16', 'outT_bf16'):
            if name in g:
                assert same_bits(g[name], f_full[i][name]), (cid, i, name)
        P.prep_bwd(outs)
    launch_bwd(nv, prod)
    for i, P in enumerate(prod):
        check_bwd(P, f'{cid}[{i}] bf16 only', full=b_full[i])


@pytest.mark.parametrize('zid', list(bu.ZERO_CASES))
def test_exact_zero_preactivation_takes_the_slope(nv, zid):
    """y > 0 is strict in every backward kernel: a column whose pre-activation is exactly 0 (constant input, beta = 0; exact on
    the device as on the host) is multiplied by the slope, and is held to the same bounds as every other column."""
    d, z = bu.zero_case_data(zid), bu.ZERO_COLUMN
    probs = [Prob(nv, d, 'f')]
    launch_fwd(nv, probs)
    g = check_fwd(probs[0], zid)
    assert float(g['out'][:, z].abs().max()) == 0
    probs[0].prep_bwd('f')
    launch_bwd(nv, probs)
    b = check_bwd(probs[0], zid)
    ref = d['ref']
    e = abs(float(b['dbeta'][z]) - float(ref['dbeta'][z])) / float(ref['abs_dd'][z])
    print(zid, f'dbeta of the zero column {e:.2e}')
    assert e <= bu.BOUND['db']


@pytest.mark.parametrize('cid', bu.ACCUMULATE_CASES)
def test_backward_accumulates_and_takes_no_dbias(nv, cid):
    """accumulate = 1 onto random previous dgamma / dbeta / dbias; dbias_lin = NULL leaves the other outputs as they were."""
    outs = bu.CASES[cid]['outs']
    probs = make_probs(nv, cid, outs)
    launch_fwd(nv, probs)
    P = probs[0]
    P.prep_bwd(outs, accumulate=True)
    launch_bwd(nv, probs)
    check_bwd(P, f'{cid} accumulate')
    P.prep_bwd(outs)
    launch_bwd(nv, probs)
    a = check_bwd(P, f'{cid} plain')
    a = {k: v.clone() for k, v in a.items()}
    P.prep_bwd(outs, dbias=False)
    launch_bwd(nv, probs)
    b = check_bwd(P, f'{cid} no dbias')
    assert set(a) - set(b) == {'dbias'}
    for k in b:
        assert same_bits(a[k], b[k]), (cid, k)


# ------------------------------------------------------------------------------------------------
# the dropout mask, bit for bit
# ------------------------------------------------------------------------------------------------
def read_mask(nv, cid, seed=bu.SEED, step=bu.STEP, dstream=0):
    """One forward launch with gamma = 0, beta = 1: out is exactly 1 / (1 - p) where the element is kept and 0 elsewhere."""
    case = bu.CASES[cid]
    probs = [Prob(nv, d, 'f', readout=True, stream=d['stream'] + dstream, offset=case.get('offset', 0))
             for d in bu.case_data(cid)]
    launch_fwd(nv, probs, rng_state(seed, step))
    P, d = probs[0], probs[0].d
    out = P.out[:d['B'] * d['N']].reshape(d['B'], d['N']).cpu()
    scale = float(np.float32(1) / (np.float32(1) - np.float32(case['p'])))
    assert bool(((out == 0) | (out == scale)).all()), cid
    return out != 0


@pytest.mark.parametrize('cid', bu.READOUT_CASES)
def test_mask_equals_host_philox(nv, cid):
    """Each forward instance draws the host's mask, element for element, and follows seed, step (both 32-bit halves) and stream."""
    d = bu.case_data(cid)[0]
    B, N, p, stream = d['B'], d['N'], d['p'], d['stream']
    base = bu.keep_mask(bu.SEED, bu.STEP, stream, B, N, p)
    assert torch.equal(base, d['keep'])
    got = read_mask(nv, cid)
    print(cid, 'keep rate', float(got.double().mean()), 'expected', bu.keep_rate(p), 'mismatches', int((got != base).sum()))
    assert torch.equal(got, base), (cid, int((got != base).sum()))
    for seed, step, ds in [(bu.SEED, bu.STEP + 1, 0), (bu.SEED, bu.STEP | (3 << 32), 0), (bu.SEED ^ (1 << 45), bu.STEP, 0),
                           (bu.SEED ^ 1, bu.STEP, 0), (bu.SEED, bu.STEP, 1)]:
        want = bu.keep_mask(seed, step, stream + ds, B, N, p)
        assert float((want != base).double().mean()) > 0.2                  # (a different mask on the host ...)
        assert torch.equal(read_mask(nv, cid, seed, step, ds), want), (cid, hex(seed), hex(step), ds)      # (... and the same one here)


def test_forward_and_backward_of_different_instances_agree(nv):
    """Case 10 is case 3 with h and da 4 bytes into their allocations, which sends it to the dword kernels: the two draw the
    same mask, and a float4 forward followed by a dword backward on the same saved statistics meets the backward bounds."""
    a, b = read_mask(nv, 'c03_production'), read_mask(nv, 'c10_misaligned')
    assert torch.equal(a, b) and torch.equal(a, bu.case_data('c03_production')[0]['keep'])
    cid = 'c03_production'
    probs = make_probs(nv, cid, 'fbt')
    launch_fwd(nv, probs)
    P = probs[0]
    check_fwd(P, 'mixed: float4')
    P.prep_bwd('fb', offset=1)                       # da misaligned: the launcher takes bn_act_bwd_kernel<true>
    launch_bwd(nv, probs)
    check_bwd(P, 'mixed: float4 forward, dword')
    # and the other way round: dword forward, float4 backward
    cid = 'c10_misaligned'
    probs = make_probs(nv, cid, 'f')
    launch_fwd(nv, probs)
    P = probs[0]
    check_fwd(P, 'mixed: dword')
    P.h = P.h[:P.one].clone()                        # the summed pre-activation in an aligned buffer: the float4 kernel takes it
    P.prep_bwd('fbt', offset=0)
    launch_bwd(nv, probs)
    check_bwd(P, 'mixed: dword forward, float4')


# ------------------------------------------------------------------------------------------------
# the column-sum rider
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cid', bu.RIDER_CASES)
def test_colsum_rider_against_fp64_and_changes_nothing(nv, cid):
    """jamie_bn_act_bwd_cs: two column-sum problems (one of three slabs a stride apart, NaN between) ride in the backward launch
    (extra workgroups of the float4 kernels; a launch of jamie_colsum_group behind the dword ones).  The sums are held to the
    dbeta bound -- sums of 130 and 512 fp32 terms per column, the lengths that bound was measured on -- and the BatchNorm
    outputs are the bits of the launch without the rider."""
    g = torch.Generator().manual_seed(77)
    x1, x2 = torch.randn(3, 130, 50, generator=g) * 3 + 1, torch.randn(1, 512, 264, generator=g)
    X1, stride1, one1 = slab_buffer(x1, False, 0, 16)
    X2 = dev(x2[0])
    o1, o2 = nanbuf(50 + 8), nanbuf(264 + 8)
    items = []
    for X, o, M, N, S, st in ((X1, o1, 130, 50, 3, stride1), (X2, o2, 512, 264, 1, 0)):
        q = nv.ColsumProblem()
        q.X, q.out, q.M, q.N, q.ld, q.nslab, q.slab_stride, q.accumulate = nv.ptr(X), nv.ptr(o), M, N, N, S, st, 0
        items.append(q)
    arr = (nv.ColsumProblem * 2)(*items)
    outs = 'fbt'
    probs = make_probs(nv, cid, outs)
    launch_fwd(nv, probs)
    P = probs[0]
    P.prep_bwd(outs)
    launch_bwd(nv, probs)
    a = {k: v.clone() for k, v in check_bwd(P, f'{cid} plain').items()}
    P.prep_bwd(outs)
    launch_bwd(nv, probs, colsums=(arr, 2, 0))
    b = check_bwd(P, f'{cid} rider')
    for k in a:
        assert same_bits(a[k], b[k]), (cid, k)
    for o, x in ((o1, x1), (o2, x2)):
        n = x.shape[2]
        assert tail_is_nan(o, n)
        e = bu.e_col(o[:n], x.double().sum((0, 1)), x.double().abs().sum((0, 1)))
        print(cid, 'column sums', tuple(x.shape), f'{e:.2e}')
        assert e <= bu.BOUND['db'], (cid, e)


# ------------------------------------------------------------------------------------------------
# argument errors
# ------------------------------------------------------------------------------------------------
def test_bad_arguments_fail_loudly(nv):
    def problem(B, N, outs, panel=False):
        d = dict(bu.make_problem(B, N, 1, 1), stream=0)
        return Prob(nv, d, outs, panel=panel)
    state = rng_state()
    with pytest.raises(nv.JamieHipError):            # bf16 output with B % 8 != 0
        nv.bn_act_fwd([problem(12, 8, 'fb').fwd_problem()], 0.0, state)
    with pytest.raises(nv.JamieHipError):            # transposed bf16 with 512 < B <= 1024 off the float4 path
        nv.bn_act_fwd([problem(520, 9, 'ft').fwd_problem()], 0.0, state)
    with pytest.raises(nv.JamieHipError):            # panels with N % 4 != 0
        nv.bn_act_fwd([problem(16, 18, 'f', panel=True).fwd_problem()], 0.0, state)
    with pytest.raises(nv.JamieHipError):            # p > 0, no mask, no rng state
        nv.bn_act_fwd([problem(16, 8, 'f').fwd_problem()], 0.5, None)
    P = problem(16, 8, 'f')
    P.prep_bwd('f')
    with pytest.raises(nv.JamieHipError):
        nv.bn_act_bwd([P.bwd_problem()], 0.5, None)
    P = problem(12, 8, 'f')
    P.prep_bwd('fb')
    with pytest.raises(nv.JamieHipError):
        nv.bn_act_bwd([P.bwd_problem()], 0.0, state)
    torch.cuda.synchronize()

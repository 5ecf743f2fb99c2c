"""What the GPU BatchNorm tests (tests/test_hip_bn.py) rest on, checked on the CPU: the host Philox against the Random123
known-answer vectors, the keep rule's rate and structure, the float32 restatement that fixes the GPU bounds, and the share of
columns the LeakyReLU kink takes out of the backward comparisons."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_util as bu  # noqa: E402

KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def test_philox_known_answers():
    """The three vectors of Random123's kat_vectors for philox4x32, 10 rounds; one by one and as one vectorised call."""
    for ctr, key, want in KAT:
        assert tuple(int(w) for w in bu.philox4x32_10(ctr, key)) == want
    ctr = [np.array([k[0][i] for k in KAT], dtype=np.uint64) for i in range(4)]
    key = [np.array([k[1][i] for k in KAT], dtype=np.uint64) for i in range(2)]
    got = bu.philox4x32_10(ctr, key)
    for j, (_, _, want) in enumerate(KAT):
        assert tuple(int(w[j]) for w in got) == want


def test_keep_rule_follows_its_contract():
    """keep_mask element by element against the docstring's formula evaluated with scalar calls; the threshold; the rate."""
    assert bu.drop_threshold(0.6) == 39321 and bu.drop_threshold(0.25) == 16384 and bu.drop_threshold(0.0) == 0
    assert bu.drop_threshold(0.9999999) == 65535
    assert abs(bu.keep_rate(0.6) - 0.4000092) < 5e-8 and bu.keep_rate(0.25) == 0.75
    seed, step, stream, B, N, p = 0xFEDCBA9876543210, (7 << 32) | 9, 11, 600, 24, 0.6
    m = bu.keep_mask(seed, step, stream, B, N, p)
    thr = bu.drop_threshold(p)
    for row, col in [(0, 0), (5, 3), (127, 4), (128, 4), (129, 23), (255, 7), (256, 0), (300, 13), (383, 9), (384, 9), (599, 23)]:
        rk = (row & 127) | ((row >> 8) << 7)
        w = bu.philox4x32_10((rk, col >> 2, stream, step & 0xFFFFFFFF), (seed & 0xFFFFFFFF, (seed >> 32) ^ (step >> 32)))
        half = (int(w[col & 3]) >> (16 * ((row >> 7) & 1))) & 0xFFFF
        assert bool(m[row, col]) == (half >= thr), (row, col)
    # the rate: 1 - thr / 65536 within 5 standard deviations of a binomial count, and NOT 1 - p to the same accuracy
    big = bu.keep_mask(seed, step, stream, 1024, 4096, p)
    n = big.numel()
    rate, want = float(big.double().mean()), bu.keep_rate(p)
    assert abs(rate - want) < 5 * (want * (1 - want) / n) ** 0.5, (rate, want)
    # every argument matters, the high words of seed and step included
    for other in [bu.keep_mask(seed ^ (1 << 40), step, stream, B, N, p), bu.keep_mask(seed, step ^ (1 << 32), stream, B, N, p),
                  bu.keep_mask(seed, step + 1, stream, B, N, p), bu.keep_mask(seed, step, stream + 1, B, N, p)]:
        assert 0.3 < float((other != m).double().mean()) < 0.7
    # rows 128 apart share a Philox call but not a half-word
    assert 0.3 < float((m[:128] != m[128:256]).double().mean()) < 0.7


def test_fp32_restatement_stays_below_the_recorded_errors():
    """bn_ref in float32 against bn_ref in float64 over the whole case table and the accumulating variants: the maxima are the
    constants F32_E of bn_util.py (rounded up to two digits), and the GPU bounds are 4 times them."""
    worst = {}
    for cid in bu.CASES:
        for i, d in enumerate(bu.case_data(cid)):
            for acc in ((False, True) if cid in bu.ACCUMULATE_CASES else (False,)):
                e = bu.restatement_errors(d, acc)
                print(cid, i, 'acc' if acc else '', ' '.join(f'{k} {v:.2e}' for k, v in e.items()))
                for k, v in e.items():
                    kind = bu.KIND[k]
                    if v > worst.get(kind, (0, ''))[0]:
                        worst[kind] = (v, f'{cid}[{i}] {k}')
    print('float32 restatement against float64:', worst)
    for kind, const in bu.F32_E.items():
        assert worst[kind][0] <= const, (kind, worst[kind], const)
        assert worst[kind][0] >= 0.8 * const, (kind, worst[kind], const)      # the constants are the measurement, not a cap
    assert bu.BOUND == {k: 4 * v for k, v in bu.F32_E.items()}
    assert bu.KINK == 2 * 4 * bu.F32_E['y']


@pytest.mark.parametrize('cid', list(bu.CASES))
def test_few_columns_sit_on_the_leaky_relu_kink(cid):
    """From the reference alone: at most 5 % of a case's columns are left out of the backward comparisons, none where
    N < 100; the constant column is exact (variance 0, y = beta = +-0.5) and so never among them."""
    for d in bu.case_data(cid):
        n_out = int(d['kink'].sum())
        print(cid, d['B'], d['N'], 'columns left out:', n_out)
        assert n_out <= bu.MAX_KINK_SHARE * d['N']
        if d['N'] < 100:
            assert n_out == 0
        if d['N'] >= 16:
            c, ref = d['const'], d['ref']
            assert float(ref['y'][:, c].abs().min()) == 0.5 and float(ref['y'][:, c].abs().max()) == 0.5
            assert abs(float(ref['save_invstd'][c]) * bu.given(d['hyper']['eps']) ** 0.5 - 1) < 1e-12
            assert float(ref['abs_ddxn'][c]) == 0 and not bool(d['kink'][c])
        else:
            assert d['const'] is None


@pytest.mark.parametrize('zid', list(bu.ZERO_CASES))
def test_exact_zero_column_is_exact_in_both_precisions(zid):
    """The column with y = 0 exactly: 0 in float64 and in float32, the slope taken (dd = slope * scale * da where kept), no
    other column on the kink, and the restatement within the recorded errors with that column taking part."""
    d, z = bu.zero_case_data(zid), bu.ZERO_COLUMN
    r32 = bu.bn_ref(d['hs'], d['gamma'], d['beta'], d['keep'], d['p'], d['das'], d['rm0'], d['rv0'], dtype=torch.float32)
    ref = d['ref']
    assert float(ref['y'][:, z].abs().max()) == 0 and float(r32['y'][:, z].abs().max()) == 0
    want = torch.where(d['keep'][:, z], d['das'][0, :, z].double() * bu.given(0.01) / (1 - 0.25), torch.zeros(d['B'], dtype=torch.float64))
    assert abs(float(ref['dbeta'][z]) - float(want.sum())) <= 1e-12 * float(want.abs().sum())
    assert int(d['kink'].sum()) == 1 and bool(d['kink'][z]) and bool(d['cols'].all())
    e = bu.restatement_errors(d)
    print(zid, ' '.join(f'{k} {v:.2e}' for k, v in e.items()))
    for k, v in e.items():
        assert v <= bu.F32_E[bu.KIND[k]], (zid, k, v)


def test_panel_helpers_round_trip():
    t = torch.arange(2 * 5 * 20, dtype=torch.float32).reshape(2, 5, 20)
    flat = bu.to_panels(t, 16, float('nan'))
    assert flat.shape == (2, 2 * 16 * 5)
    assert float(flat[0, (1 * 5 + 3) * 16 + 2]) == float(t[0, 3, 18])             # ((col // P) * B + row) * P + col % P
    back, pad = bu.from_panels(flat, 5, 20, 16)
    assert torch.equal(back, t) and pad.shape == (2, 5, 12) and bool(torch.isnan(pad).all())

"""What the GPU batch-assembly tests (tests/test_hip_assembly.py) rest on, checked on the CPU: the host restatement of the
device sampler (tests/sampler_util.py: choice, rand4, hybrid).  The GPU tests compare the kernels with it index for index;
here the restatement itself is held to the contract that the header of csrc/sampler.h states -- B distinct values of the
range, every B-subset equally likely and in uniformly random order, streams and steps independent -- over as many steps
as the statistics need.  All seeds are fixed: nothing here can flake."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_util as bu  # noqa: E402
import sampler_util as su  # noqa: E402

SEED = 20240607


def test_rand4_is_philox_on_the_documented_counter_and_key():
    """rand4 against philox4x32_10 on hand-written counters and keys; seed, step and idx4 above 2^32; vectorised = scalar."""
    cases = [
        # seed, step, stream, idx4 -> counter, key
        (7, 0, 200, 0, (0, 0, 200, 0), (7, 0)),
        (0x1_0000_0007, 5, 3, 0x1234, (0x1234, 0, 3, 5), (7, 1)),
        (0xABCD_0000_0011, (9 << 32) | 2, 203, (3 << 32) | 0x80, (0x80, 3, 203, 2), (0x11, 0xABCD ^ 9)),
        (0xFFFF_FFFF_FFFF_FFFF, 0xFFFF_FFFF_0000_0001, 0xFFFF_FFFF, 0xFFFF_FFFF_FFFF_FFFF,
         (0xFFFF_FFFF, 0xFFFF_FFFF, 0xFFFF_FFFF, 1), (0xFFFF_FFFF, 0)),
    ]
    for seed, step, stream, idx4, ctr, key in cases:
        got = tuple(int(w) for w in su.rand4(seed, step, stream, idx4))
        assert got == tuple(int(w) for w in bu.philox4x32_10(ctr, key)), (seed, step, stream, idx4)
    idx = np.array([0, 1, 0x1234, (3 << 32) | 0x80], dtype=np.uint64)
    vec = su.rand4(0xABCD_0000_0011, (9 << 32) | 2, 203, idx)
    for j, i in enumerate(idx):
        assert tuple(int(w[j]) for w in vec) == tuple(int(w) for w in su.rand4(0xABCD_0000_0011, (9 << 32) | 2, 203, int(i)))
    # every argument matters, the high words included
    base = tuple(int(w) for w in su.rand4(5, 6, 7, 8))
    for other in [(5 | 1 << 40, 6, 7, 8), (5, 6 | 1 << 40, 7, 8), (5, 6, 8, 8), (5, 6, 7, 8 | 1 << 40), (5, 7, 7, 8)]:
        assert tuple(int(w) for w in su.rand4(*other)) != base


@pytest.mark.parametrize('N,B,offset', [(1, 1, 0), (5, 3, 9), (48, 48, 2), (2048, 2048, 3), (4096, 1, 0), (4096, 2048, 0),
                                        (4096, 4, 5), (4097, 1, 0), (4097, 2048, 0), (4097, 1025, 7), (5000, 1024, 0),
                                        (2 ** 31 - 12, 2048, 11)])
def test_draws_without_replacement_are_distinct_and_in_range(N, B, offset):
    """Both methods (N <= 4096 sort, N > 4096 claim): a permutation (N = B), the method switch 4096 / 4097, B = 1, the
    largest B and the largest N + offset; three steps each."""
    for step in (0, 1, 2 ** 32 + 5):
        v = su.choice(SEED, step, 200, B, N, offset, False)
        assert v.shape == (B,) and v.dtype == np.int64
        assert np.unique(v).size == B and v.min() >= offset and v.max() < offset + N
    if N == B:
        assert np.array_equal(np.sort(v), np.arange(offset, offset + N))


def test_draws_with_replacement_follow_their_formula():
    v = su.choice(SEED, 3, 201, 700, 100, 4, True)
    assert v.min() >= 4 and v.max() < 104 and np.unique(v).size < 700
    for s in (0, 1, 699):
        w = su.rand4(SEED, 3, 201, s << 8)
        assert v[s] == ((int(w[0]) << 32) | int(w[1])) % 100 + 4


def test_sort_method_is_the_b_smallest_keys_in_key_order():
    """The sort method restated once more with Python integers and sorted(): key = ((v0 >> 1) << 32) | candidate."""
    N, B, off = 37, 11, 5
    keys = []
    for i in range(N):
        v0 = int(su.rand4(SEED, 9, 202, i << 8)[0])
        keys.append((((v0 >> 1) << 32) | i, i))
    want = [i + off for _, i in sorted(keys)[:B]]
    assert su.choice(SEED, 9, 202, B, N, off, False).tolist() == want


def test_claim_method_follows_its_rules_slot_by_slot():
    """The claim method restated once more with a Python loop, a set and scalar rand4 calls, at N = 4097, B = 1100 (two
    chunks, many redraws): a draw is accepted iff no slot accepted in an earlier round or chunk holds the value and it has
    the lowest slot number among the round's draws of the value."""
    N, B, step, stream = 4097, 1100, 2 ** 32 + 5, 203
    held, out = set(), [None] * B
    for base in range(0, B, 1024):
        todo = list(range(base, min(base + 1024, B)))
        for rnd in range(64):
            w = su.rand4(SEED, step, stream, np.array([(s << 8) | rnd for s in todo], dtype=np.uint64))
            draw = [((int(a) << 32) | int(b)) % N for a, b in zip(w[0], w[1])]
            first, nxt = {}, []
            for s, d in zip(todo, draw):
                out[s] = d
                first.setdefault(d, s)
            for s, d in zip(todo, draw):
                if d in held or first[d] != s:
                    nxt.append(s)
            held.update(d for s, d in zip(todo, draw) if s not in set(nxt))
            todo = nxt
            if not todo:
                break
        assert not todo
    assert su.choice(SEED, step, stream, B, N, 0, False).tolist() == out


# ------------------------------------------------------------------------------------------------
# uniform subsets in uniform order
# ------------------------------------------------------------------------------------------------
def test_sort_method_arrangements_are_equally_frequent():
    """(a) N = 5, B = 3: the 60 ordered arrangements over T = 6000 steps (expected count 100 each), Pearson chi-square with
    59 degrees of freedom against its 1 - 1e-6 quantile.
    Reached: statistic 70.70, bound 125.66."""
    N, B, T = 5, 3, 6000
    arrangements = {p: k for k, p in enumerate(itertools.permutations(range(N), B))}
    assert len(arrangements) == 60
    counts = np.zeros(60)
    for step in range(T):
        counts[arrangements[tuple(su.choice(SEED, step, 200, B, N, 0, False).tolist())]] += 1
    stat, bound = su.pearson(counts, np.full(60, T / 60)), su.chi2_bound(59)
    print(f'SAMPLER (a) N={N} B={B} T={T}: chi2 {stat:.2f} bound {bound:.2f}')
    assert T / 60 >= 20 and stat < bound, (stat, bound)


def test_claim_method_is_uniform_at_its_worst_collision_rate():
    """(b) N = 4097, B = 2048 over T = 200 steps.  Every step puts each cell into one of five states -- left out, or at a slot
    of (chunk 0 | 1) x (even | odd slot), 512 slots each -- and into one of two, in or out; both tables against
    sampler_util.assignment_chi2 (Pearson, scaled by (N - 1) / N, (N - 1)(K - 1) degrees of freedom).  The smallest expected
    count is 200 * 512 / 4097 = 24.99.
    Reached: inclusion 4011.21 (bound 4540.72, 4096 degrees of freedom); chunk x parity 16238.29 (bound 17258.90, 16384
    degrees of freedom); the restatement needed up to 19 rounds."""
    N, B, T = 4097, 2048, 200
    table = np.zeros((N, 5))
    state_of_slot = 1 + 2 * (np.arange(B) // 1024) + (np.arange(B) & 1)
    worst = 0
    for step in range(T):
        v, rounds = su.choice(SEED, step, 200, B, N, 0, False, with_rounds=True)
        worst = max(worst, rounds)
        row = np.zeros(N, dtype=np.int64)
        row[v] = state_of_slot
        table[np.arange(N), row] += 1
    incl = np.stack([table[:, 0], table[:, 1:].sum(1)], axis=1)
    s2, dof2, e2 = su.assignment_chi2(incl, [N - B, B], T)
    s5, dof5, e5 = su.assignment_chi2(table, [N - B, 512, 512, 512, 512], T)
    b2, b5 = su.chi2_bound(dof2), su.chi2_bound(dof5)
    print(f'SAMPLER (b) N={N} B={B} T={T}: inclusion chi2 {s2:.2f} bound {b2:.2f} dof {dof2}; chunk x parity chi2 {s5:.2f} '
          f'bound {b5:.2f} dof {dof5}; smallest expected {e5:.2f}; rounds <= {worst}')
    assert min(e2, e5) >= 20 and worst < 64
    assert s2 < b2 and s5 < b5, (s2, b2, s5, b5)


def test_claim_method_does_not_bias_late_slots():
    """(c) N = 5000, B = 1500 over T = 400 steps: the mean index per slot does not depend on the slot
    (sampler_util.slot_mean_chi2, 1500 degrees of freedom), and -- on exact counts -- every slot holds an index of the lower
    half of the range in half of the steps: per slot a binomial(T, 1/2) count, expected 200, so sum (O - T/2)^2 / (T/4) over
    the slots has 1500 degrees of freedom (the slots of one step are negatively correlated, covariance -1 / (4 (N - 1)),
    which moves the statistic by a factor within 1 +- B / N of 1 on one direction out of 1500 only).  A slot that loses a
    round redraws, so a bias of redrawn slots would show in both.
    Reached: slot means 1451.62, lower half 1489.13, bound 1774.90."""
    N, B, T = 5000, 1500, 400
    sums, low = np.zeros(B), np.zeros(B)
    for step in range(T):
        v = su.choice(SEED, step, 200, B, N, 0, False)
        sums += v
        low += v < N // 2
    stat, dof = su.slot_mean_chi2(sums, T, N)
    stat_low = float(((low - T / 2) ** 2 / (T / 4)).sum())
    bound = su.chi2_bound(dof)
    print(f'SAMPLER (c) N={N} B={B} T={T}: slot-mean chi2 {stat:.2f}, lower-half chi2 {stat_low:.2f}, bound {bound:.2f} dof {dof}')
    assert dof == B and T / 2 >= 20
    assert stat < bound and stat_low < bound, (stat, stat_low, bound)


# ------------------------------------------------------------------------------------------------
# streams and steps
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,B', [(1536, 128), (5000, 1500), (100_000, 512)])
def test_streams_and_steps_are_independent_and_step_add_is_a_step(N, B):
    """`step - 1` with step_add = 1 is `step`, exactly.  Streams 200..203 at one step and steps 7, 8, 2^32 + 7 at one stream
    are seven draws; each of their 21 pairs shares at most sampler_util.overlap_bound values: the hypergeometric(N, B, B)
    quantile at 1e-6 / 21, i.e. the mean B^2 / N plus the margin that this union bound gives (N = 1536: mean 10.7, bound 29, reached 15;
    N = 5000: mean 450, bound 530, reached 468; N = 100 000: mean 2.6, bound 15, reached 6).  The same slot holds the same value in at most 6 places:
    the count is at most binomial-like with mean B / N <= 0.3, and P(Poisson(0.3) > 6) < 1e-8."""
    step = 8
    a = su.choice(SEED, step, 200, B, N, 3, False)
    assert np.array_equal(a, su.choice(SEED, step - 1, 200, B, N, 3, False, step_add=1))
    assert np.array_equal(su.choice(SEED, 2 ** 32, 200, B, N, 3, False), su.choice(SEED, 2 ** 32 - 1, 200, B, N, 3, False, step_add=1))
    draws = [su.choice(SEED, step, s, B, N, 3, False) for s in (200, 201, 202, 203)]
    draws += [su.choice(SEED, s, 200, B, N, 3, False) for s in (7, 2 ** 32 + 7, 2 ** 32 + 8)]
    pairs = list(itertools.combinations(range(len(draws)), 2))
    bound, mean = su.overlap_bound(N, B, len(pairs))
    worst = max(np.intersect1d(draws[i], draws[j]).size for i, j in pairs)
    same_place = max(int((draws[i] == draws[j]).sum()) for i, j in pairs)
    print(f'SAMPLER overlap N={N} B={B}: worst {worst}, mean {mean:.1f}, bound {bound}; same slot and value {same_place}')
    assert worst <= bound and same_place <= 6
    # with replacement too
    r = [su.choice(SEED, step, s, B, N, 0, True) for s in (200, 201)]
    assert int((r[0] == r[1]).sum()) <= 6


# ------------------------------------------------------------------------------------------------
# the cases of the GPU comparison
# ------------------------------------------------------------------------------------------------
def test_gpu_cases_need_many_rounds_but_never_all():
    """Rounds that the claim method runs for the cases of tests/test_hip_assembly.py (largest over the three steps):
    f 16, g 6, h 5, i 2, j 1.  At least one case needs >= 6 (the redraw rounds run), none needs 64 (no slot is left
    unresolved: choice asserts that as well)."""
    rounds = {}
    for cid, (N, B, off, rep) in su.SAMPLER_CASES.items():
        worst = 0
        for step in su.STEPS:
            v, r = su.choice(su.SEED, step, su.STREAM, B, N, off, rep, with_rounds=True)
            worst = max(worst, r)
            assert v.min() >= off and v.max() < off + N and (rep or np.unique(v).size == B)
        rounds[cid] = worst
    print('SAMPLER rounds', rounds)
    assert max(rounds.values()) >= 6 and max(rounds.values()) < 64
    assert all((r > 0) == (not su.SAMPLER_CASES[c][3] and su.SAMPLER_CASES[c][0] > su.SORT_MAX) for c, r in rounds.items())


def test_hybrid_pairs_the_slots_below_the_ratio():
    """hybrid against a scalar loop; true_ratio 0, 0.8 and 1; num_corr 0; the modulo on pair numbers; and the draw that rounds
    to x = 1.0 in float32 (seed 0x1_0000_0007, stream 204, step 4755, slot 1807: v0 = 0xFFFFFF98), which true_ratio = 1 pairs
    like every other slot."""
    B, nc = 300, 7
    g = np.random.default_rng(3)
    pairs = g.integers(0, 1000, (nc, 2))
    pidx, r0, r1 = g.integers(0, 50, B), g.integers(0, 1000, B), g.integers(0, 1000, B)
    for tr in (0.0, 0.8, 1.0):
        i0, i1, paired = su.hybrid(SEED, 4, 204, pairs, pidx, r0, r1, nc, tr)
        for b in range(B):
            x = np.float32(int(su.rand4(SEED, 4, 204, b)[0])) * np.float32(2.0 ** -32)
            p = bool(x < np.float32(tr)) or tr >= 1
            assert paired[b] == p
            assert (i0[b], i1[b]) == ((pairs[pidx[b] % nc][0], pairs[pidx[b] % nc][1]) if p else (r0[b], r1[b]))
        assert abs(paired.mean() - tr) < 0.1
    i0, i1, paired = su.hybrid(SEED, 4, 204, None, pidx, r0, r1, 0, 0.8)
    assert not paired.any() and np.array_equal(i0, r0) and np.array_equal(i1, r1)
    assert int(su.rand4(0x1_0000_0007, 4755, 204, 1807)[0]) == 0xFFFFFF98
    x = su.hybrid_x(0x1_0000_0007, 4755, 204, 2048)
    assert x[1807] == np.float32(1.0) and (x < 1).sum() == 2047
    assert su.hybrid(0x1_0000_0007, 4755, 204, pairs, np.zeros(2048), np.ones(2048), np.ones(2048), nc, 1.0)[2].all()

"""Shared by tests/test_host_sampler.py and tests/test_hip_assembly.py: a host restatement of the device sampler
(csrc/sampler.h, the device `np.random.choice`) and of the hybrid batch assembly (hybrid_assemble_kernel, csrc/misc.hip),
the chi-square statistics that the uniformity claims are checked with, and the error bound of a row-normalised block.
numpy only; no GPU code.

The restatement states the CONTRACT of sampler.h, not its mechanism: no hash table, no bitonic network, no atomics.  Where
it and a kernel disagree, the kernel is wrong unless the restatement misreads the header of sampler.h."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bn_util import philox4x32_10  # noqa: E402

MASK32 = (1 << 32) - 1
MASK64 = (1 << 64) - 1
SORT_MAX = 4096          # SMP_HASH: N <= 4096 takes the sort method, larger N the claim method
CHUNK = 1024             # slots of the claim method that draw together
ROUNDS = 64              # redraw rounds of a chunk
MAX_B = 2048             # largest B without replacement (SMP_HASH / 2)
U64 = np.uint64


def rand4(seed, step, stream, idx4):
    """jamie_rand4 (csrc/common.h): four 32-bit words (uint64 arrays) of Philox4x32-10 with
    counter = (low 32 bits of idx4, high 32 bits of idx4, stream, low 32 bits of step) and
    key = (low 32 bits of seed, high 32 bits of seed XOR high 32 bits of step).  idx4: int or uint64 array."""
    seed, step = int(seed) & MASK64, int(step) & MASK64
    idx4 = np.asarray(idx4, dtype=U64)
    return philox4x32_10((idx4 & U64(MASK32), idx4 >> U64(32), U64(int(stream) & MASK32), U64(step & MASK32)),
                         (U64(seed & MASK32), U64((seed >> 32) ^ (step >> 32))))


def _draw(seed, step, stream, idx4, N):
    """(v0 << 32 | v1) mod N of rand4(idx4): int64 array."""
    v = rand4(seed, step, stream, idx4)
    return (((v[0] << U64(32)) | v[1]) % U64(N)).astype(np.int64)


def choice(seed, step, stream, B, N, offset, replace, step_add=0, with_rounds=False):
    """The B indices (int64 array) that the device sampler writes for (seed, step + step_add, stream): B values of
    [offset, offset + N), distinct unless `replace`.  `with_rounds`: also the number of rounds that the claim method ran
    (the largest over its chunks; 0 for the other methods)."""
    B, N, offset = int(B), int(N), int(offset)
    assert B >= 1 and N >= 1 and N + offset <= 2 ** 31 - 1 and (replace or (B <= N and B <= MAX_B))
    step = (int(step) + int(step_add)) & MASK64
    rounds = 0
    if replace:
        out = _draw(seed, step, stream, np.arange(B, dtype=U64) << U64(8), N)
    elif N <= SORT_MAX:
        # every candidate gets a 31-bit random key, ties broken by the candidate's number; the B smallest, in key order
        cand = np.arange(N, dtype=U64)
        key = ((rand4(seed, step, stream, cand << U64(8))[0] >> U64(1)) << U64(32)) | cand
        out = np.argsort(key, kind='stable')[:B].astype(np.int64)
    else:
        out = np.full(B, -1, dtype=np.int64)
        held = np.empty(0, dtype=np.int64)                         # the values of every accepted slot so far
        for base in range(0, B, CHUNK):
            todo = np.arange(base, min(base + CHUNK, B), dtype=U64)       # the unresolved slots, ascending
            for rnd in range(ROUNDS):
                draw = _draw(seed, step, stream, (todo << U64(8)) | U64(rnd), N)
                out[todo.astype(np.int64)] = draw                  # (a slot unresolved after the last round keeps this)
                lowest = np.zeros(draw.size, dtype=bool)
                lowest[np.unique(draw, return_index=True)[1]] = True       # first occurrence = lowest slot number
                ok = lowest & ~np.isin(draw, held)
                held = np.concatenate([held, draw[ok]])
                todo = todo[~ok]
                if todo.size == 0:
                    break
            rounds = max(rounds, rnd + 1)
            assert todo.size == 0, f'{todo.size} slots unresolved after {ROUNDS} rounds (N={N}, B={B}, step={step})'
    out = out + offset
    return (out, rounds) if with_rounds else out


def hybrid_x(seed, step, stream, B):
    """The uniform number of slot b as the kernel forms it, in float32: float32(v0 of rand4(idx4 = b)) * float32(2^-32).
    The conversion rounds to nearest, so v0 >= 0xFFFFFF80 gives 1.0."""
    v0 = rand4(seed, step, stream, np.arange(B, dtype=U64))[0]
    return v0.astype(np.float32) * np.float32(2.0 ** -32)


def hybrid(seed, step, stream, pairs, pidx, r0, r1, num_corr, true_ratio):
    """hybrid_assemble_kernel: slot b is paired iff num_corr > 0 and (x_b < float32(true_ratio) or true_ratio >= 1); a
    paired slot takes pair number pidx[b] mod num_corr (modality 0 its first, modality 1 its second entry), any other slot
    r0[b] and r1[b].  (true_ratio = 1 pairs every slot, like `np.random.rand() < 1` of the reference, although x_b can round
    up to 1.0.)  pairs: int array [num_corr, 2] or None.  Returns (idx0, idx1, paired)."""
    pidx, r0, r1 = (np.asarray(a, dtype=np.int64) for a in (pidx, r0, r1))
    B = pidx.size
    tr = np.float32(true_ratio)
    paired = np.zeros(B, dtype=bool)
    if num_corr > 0:
        paired = (hybrid_x(seed, step, stream, B) < tr) | bool(tr >= np.float32(1.0))
    idx0, idx1 = r0.copy(), r1.copy()
    if paired.any():
        k = pidx[paired] % num_corr
        pr = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        idx0[paired], idx1[paired] = pr[k, 0], pr[k, 1]
    return idx0, idx1, paired


# ------------------------------------------------------------------------------------------------
# the cases that the device sampler is compared on, index for index
# ------------------------------------------------------------------------------------------------
SEED = 0x1_0000_0007                       # both words of the seed and (last step) of the step counter are in use
STEPS = (0, 1, 2 ** 32 + 5)
STREAM = 200
# id -> (N, B, offset, replace)
SAMPLER_CASES = {
    'a_smallest': (1, 1, 0, False),
    'b_sort_padding': (5, 3, 9, False),
    'c_sort_small_data': (1536, 128, 0, False),
    'd_sort_full_table': (4096, 2048, 0, False),
    'e_sort_permutation': (2048, 2048, 3, False),
    'f_claim_two_chunks': (4097, 2048, 0, False),
    'g_claim_chunk_of_one': (4097, 1025, 0, False),
    'h_claim_one_chunk': (5000, 1024, 0, False),
    'i_existing_shape': (100_000, 512, 7, False),
    'j_largest_n': (2 ** 31 - 1 - 11, 2048, 11, False),
    'k_replace_b_above_n': (100, 700, 0, True),
    'l_replace_large': (2 ** 31 - 1, 3000, 0, True),
}
RIDER_CASES = ('c_sort_small_data', 'd_sort_full_table', 'f_claim_two_chunks', 'g_claim_chunk_of_one', 'i_existing_shape')


# ------------------------------------------------------------------------------------------------
# chi-square statistics for "a uniform subset in uniform order"
# ------------------------------------------------------------------------------------------------
P_FALSE_ALARM = 1e-6


def chi2_bound(dof):
    """The 1 - 1e-6 quantile of the chi-square distribution with `dof` degrees of freedom."""
    from scipy.stats import chi2
    return float(chi2.ppf(1.0 - P_FALSE_ALARM, dof))


def pearson(observed, expected):
    """sum (O - E)^2 / E."""
    o, e = np.asarray(observed, dtype=np.float64), np.asarray(expected, dtype=np.float64)
    return float(((o - e) ** 2 / e).sum())


def assignment_chi2(table, state_sizes, T):
    """Every one of T independent steps puts each of N cells into exactly one of K states, state k holding exactly
    state_sizes[k] cells (sum = N); under the contract every such assignment is equally likely.  `table` [N, K] counts how
    often a cell was in a state; its expectation is T * state_sizes[k] / N.  For one step the Pearson statistic of the
    one-hot table is the constant N (K - 1) (each row contributes (1 - p_k) / p_k, and state k has N p_k rows), and the
    indicator covariance under fixed margins is N / (N - 1) times the projection that the chi-square limit assumes, so
    X^2 (N - 1) / N has mean (N - 1)(K - 1) exactly and is asymptotically chi-square with (N - 1)(K - 1) degrees of
    freedom as T grows.  Returns (the scaled statistic, the degrees of freedom, the smallest expected count)."""
    table = np.asarray(table, dtype=np.float64)
    N, K = table.shape
    sizes = np.asarray(state_sizes, dtype=np.float64)
    assert sizes.sum() == N and table.sum() == T * N
    expected = np.broadcast_to(T * sizes / N, table.shape)
    return pearson(table, expected) * (N - 1) / N, (N - 1) * (K - 1), float(expected.min())


def slot_mean_chi2(sums, T, N):
    """sums[s]: the sum over T independent steps of the index at slot s of a no-replacement draw of B = len(sums) out of
    [0, N).  Under the contract the index at a slot is uniform: mean (N - 1) / 2, variance v = (N^2 - 1) / 12, and two slots
    of one step have covariance -v / (N - 1).  That covariance matrix has the eigenvalue v N / (N - 1) on the B - 1
    directions orthogonal to the all-ones vector and v (N - B) / (N - 1) on it, so with d = sums / T - (N - 1) / 2 split into
    its mean and the rest,  T |d - mean(d)|^2 / (v N / (N - 1)) + T B mean(d)^2 / (v (N - B) / (N - 1))  is (by the central
    limit theorem over the T steps) chi-square with B degrees of freedom.  Returns (statistic, B)."""
    sums = np.asarray(sums, dtype=np.float64)
    B = sums.size
    d = sums / T - (N - 1) / 2.0
    v = (N * N - 1) / 12.0
    dbar = d.mean()
    stat = T * ((d - dbar) ** 2).sum() / (v * N / (N - 1)) + T * B * dbar ** 2 / (v * (N - B) / (N - 1))
    return float(stat), B


def overlap_bound(N, B, comparisons):
    """Two independent uniform B-subsets of N cells share a hypergeometric(N, B, B) number of values, mean B^2 / N.  The
    bound is that distribution's upper quantile at 1e-6 / comparisons (a union bound over the pairs compared): the smallest
    k with P(shared > k) <= 1e-6 / comparisons.  Returns (bound, mean)."""
    from scipy.stats import hypergeom
    return int(hypergeom(N, B, B).isf(P_FALSE_ALARM / comparisons)), B * B / N


# ------------------------------------------------------------------------------------------------
# error bound of a row-normalised block (jamie_csr_block, jamie_dense_block)
# ------------------------------------------------------------------------------------------------
EPS32 = 2.0 ** -24          # unit roundoff of float32 (round to nearest)


def normalised_row_bound(abs_row_sum, row_sum, B1):
    """Relative bound on |fl(v / fl(S)) - v / S| per row, S the sum of the row's B1 gathered elements, from the standard model
    fl(a op b) = (a op b)(1 + d), |d| <= u = 2^-24:
      * fl(S) is a float32 sum of B1 terms in some tree order: |fl(S) - S| <= gamma A, gamma = (B1 - 1) u / (1 - (B1 - 1) u),
        A = sum |v| (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2: any order of summation);
      * the quotient is rounded once: one more u.
    So the bound is (gamma A / |S| + u) * 1.01 relative to |v / S|; the 1.01 covers the second-order terms (gamma A / |S| is
    below 1e-4 for the rows used).  It grows with B1 through gamma and with the cancellation A / |S| of the row.  Whatever is
    done to the quotient afterwards (a product with a weight, a second block mixed in) adds one u per rounding, relative to
    the magnitudes involved: the caller adds those.  Rows with S == 0 stay unnormalised and are exact: 0."""
    A, S = np.asarray(abs_row_sum, dtype=np.float64), np.asarray(row_sum, dtype=np.float64)
    gamma = (B1 - 1) * EPS32 / (1.0 - (B1 - 1) * EPS32)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(S == 0, 0.0, (gamma * A / np.abs(S) + EPS32) * 1.01)

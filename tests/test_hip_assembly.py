"""The kernels that decide which cells go into a training step -- csrc/sampler.h through its three launchers, and the batch
assembly and standardisation kernels of csrc/misc.hip -- against the host restatement of tests/sampler_util.py (index for
index) and against numpy / float64 (element for element).  Run on the MI355X box:  pytest -m gpu tests/test_hip_assembly.py

The sizes below sit on compile-time constants of the kernels -- a retune has to move them:
  sampler.h:             SMP_HASH = 4096: N <= 4096 takes the sort method (a 4096-entry bitonic network, padded), larger N the
                         claim method with a 4096-entry table, so B <= 2048 without replacement; slots are claimed in chunks of
                         1024 (B = 1024, 1025, 2048 are one chunk, a second chunk of one slot, two full chunks).
  launchers:             jamie_sample_indices[_group] run it with 1024 threads; the clip + Adam rider with JAMIE_ADAM_T = 512
                         (two slots per thread and chunk, a 512-stride through the sort network).
  256-thread loops:      corr_from_indices, csr_block, dense_block (one workgroup per row, columns b, b + 256, ...: B = 255,
                         256, 257 and 600 / 700), hybrid_assemble and axpby (one element per thread, 256 per workgroup).
  gather_rows:           at most 8 x 256 threads per row, one float4 each: a row of d > 8192 floats makes the float4 loop turn
                         twice (d = 8200); d mod 4 != 0 or a pointer off 16 bytes takes the scalar loop.
  col_stats:             64 columns per workgroup (d = 63, 64, 65), 4 row phases, 1 <= n_row_blocks <= 1024."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_util as su  # noqa: E402
from oracle import jamie_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINELS = 64
SENTINEL = {torch.int32: -7777, torch.float32: -7.5, torch.float64: -7.5, torch.bfloat16: -7.5}
EPS32 = su.EPS32


@pytest.fixture(scope='module')
def nv():
    from jamie_amd import _native
    _native.require_gpu()
    return _native


def buffer(shape, dtype):
    """An output buffer that holds the sentinel everywhere, with SENTINELS more elements behind it: (whole buffer, the view
    of `shape` that the kernel is given)."""
    n = int(np.prod(shape))
    full = torch.full((n + SENTINELS,), SENTINEL[dtype], dtype=dtype, device='cuda')
    return full, full[:n].view(shape)


def padded(t):
    """A device copy of `t` with SENTINELS sentinel elements behind it: (whole buffer, view of t's shape)."""
    full, view = buffer(tuple(t.shape), t.dtype)
    view.copy_(t)
    return full, view


def intact(full):
    return bool((full[-SENTINELS:] == SENTINEL[full.dtype]).all())


def untouched(full):
    return bool((full == SENTINEL[full.dtype]).all())


def rng_state(seed, step):
    """[seed, step, 0, 0] as the engine keeps it (uint64 on the device; a step of -1 is 2^64 - 1)."""
    return torch.tensor([seed, step, 0, 0], dtype=torch.int64, device='cuda')


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ------------------------------------------------------------------------------------------------
# the sampler, index for index
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def want_indices(cid, step, stream=su.STREAM, step_add=0):
    N, B, off, rep = su.SAMPLER_CASES[cid]
    return torch.from_numpy(su.choice(su.SEED, step, stream, B, N, off, rep, step_add=step_add).astype(np.int32))


@pytest.mark.parametrize('cid', list(su.SAMPLER_CASES))
def test_sampler_equals_the_restatement(nv, cid):
    """jamie_sample_indices == sampler_util.choice at steps 0, 1 and 2^32 + 5 with a seed above 2^32."""
    N, B, off, rep = su.SAMPLER_CASES[cid]
    for step in su.STEPS:
        full, idx = buffer((B,), torch.int32)
        nv.sample_indices(idx, N, off, rep, rng_state(su.SEED, step), su.STREAM)
        got = idx.cpu()
        assert torch.equal(got, want_indices(cid, step)), (cid, step, int((got != want_indices(cid, step)).sum()))
        assert intact(full)


@pytest.mark.parametrize('first', [0, 4, 8])
def test_sampler_group_equals_the_restatement(nv, first):
    """jamie_sample_indices_group: the cases four at a time, each with its own stream, the third with step_add = 1."""
    cids = list(su.SAMPLER_CASES)[first:first + 4]
    for step in su.STEPS:
        bufs = [buffer((su.SAMPLER_CASES[c][1],), torch.int32) for c in cids]
        items = []
        for k, (c, (_, idx)) in enumerate(zip(cids, bufs)):
            N, B, off, rep = su.SAMPLER_CASES[c]
            items.append(nv.sample_args(idx, N, off, rep, 200 + k, step_add=int(k == 2)))
        nv.sample_indices_group(items, rng_state(su.SEED, step))
        for k, (c, (full, idx)) in enumerate(zip(cids, bufs)):
            assert torch.equal(idx.cpu(), want_indices(c, step, 200 + k, int(k == 2))), (c, step)
            assert intact(full)


ADAM_N = 4099


def _adam_launch(nv, step, sample_of=None):
    """The norm launch and clip + Adam on a vector of 4099 parameters with the counter arriving at `step`; `sample_of`: a
    case whose draw rides in the clip + Adam launch.  Returns (parameters, moments, bf16 copy as CPU bit patterns, indices)."""
    g = torch.Generator().manual_seed(5)
    p0, gr = torch.randn(ADAM_N, generator=g), torch.randn(ADAM_N, generator=g) * 1e-3
    hyper = torch.zeros(16)
    hyper[8:14] = torch.tensor([1e-3, 0.9, 0.999, 1e-8, 1.0, 1.0])
    (pf, p), (gf, gd) = padded(p0), padded(gr)
    (mf, m), (vf, v) = padded(torch.zeros(ADAM_N)), padded(torch.zeros(ADAM_N))
    bf, pb = padded(torch.zeros(ADAM_N, dtype=torch.bfloat16))
    state = rng_state(su.SEED, step - 1)
    part = torch.zeros(nv.optim_blocks(ADAM_N), device='cuda')
    nv.grad_sqnorm(gd, part, state)                                  # the counter: step - 1 -> step
    full = idx = None
    if sample_of is None:
        nv.clip_adam(p, gd, m, v, part, hyper.cuda(), state, pb)
    else:
        N, B, off, rep = su.SAMPLER_CASES[sample_of]
        full, idx = buffer((B,), torch.int32)
        nv.clip_adam(p, gd, m, v, part, hyper.cuda(), state, pb, sample=nv.sample_args(idx, N, off, rep, su.STREAM))
    torch.cuda.synchronize()
    assert int(state[1].item()) == step and int(state[0].item()) == su.SEED
    assert all(intact(x) for x in (pf, gf, mf, vf, bf)) and (full is None or intact(full))
    return [bits(t).cpu() for t in (p, m, v, pb)], None if idx is None else idx.cpu()


@functools.lru_cache(maxsize=None)
def _adam_alone(step):
    from jamie_amd import _native
    return _adam_launch(_native, step)[0]


@pytest.mark.parametrize('cid', su.RIDER_CASES)
def test_sampler_riding_clip_adam_equals_the_restatement(nv, cid):
    """jamie_clip_adam_ride runs sampler.h with 512 threads: two slots per thread in both chunks of the claim method, a
    512-stride through the sort network.  The indices equal `choice` at the step the launch sees; parameters, moments and the
    bf16 copy equal the launch without a rider bit for bit (at step 0 Adam's bias correction is 0 and they are all NaN: the
    comparison is of bit patterns)."""
    for step in su.STEPS:
        tensors, idx = _adam_launch(nv, step, cid)
        assert torch.equal(idx, want_indices(cid, step)), (cid, step, int((idx != want_indices(cid, step)).sum()))
        for a, b in zip(tensors, _adam_alone(step)):
            assert torch.equal(a, b), (cid, step)


def test_sampler_refuses_what_it_cannot_draw(nv):
    """B > N and B = 2049 without replacement, N + offset = 2^31, B = 0 and a group of five raise and write nothing."""
    full, idx = buffer((3000,), torch.int32)
    state = rng_state(su.SEED, 1)
    refused = [(idx[:10], 5, 0, False), (idx[:2049], 100_000, 0, False), (idx[:4], 2 ** 31 - 5, 5, False),
               (idx[:4], 2 ** 31, 0, True), (idx[:4], 2 ** 31 - 5, 5, True), (idx[:0], 100, 0, False), (idx[:0], 100, 0, True)]
    for view, N, off, rep in refused:
        with pytest.raises(nv.JamieHipError):
            nv.sample_indices(view, N, off, rep, state, su.STREAM)
        with pytest.raises(nv.JamieHipError):
            nv.sample_indices_group([nv.sample_args(idx[:8], 100, 0, False, 201), nv.sample_args(view, N, off, rep, 200)], state)
    five = [nv.sample_args(idx[8 * k:8 * k + 8], 100, 0, False, 200 + k) for k in range(5)]
    with pytest.raises(nv.JamieHipError):
        nv.sample_indices_group(five, state)
    torch.cuda.synchronize()
    assert untouched(full)
    nv.sample_indices_group(five[:4], state)                  # (the same items, one fewer, are drawn)
    torch.cuda.synchronize()
    assert not untouched(full[:32]) and untouched(full[32:])


# ------------------------------------------------------------------------------------------------
# hybrid_assemble
# ------------------------------------------------------------------------------------------------
HYBRID_STREAM = 204
# found by a search over rand4(seed, step, 204, slot), slot < 2048, step = 0, 1, ...: the first draw with v0 >= 0xFFFFFF80,
# after 2^23.3 draws (expected once in 2^25); float32(v0) * 2^-32 is 1.0 there
ONE_SEED, ONE_STEP, ONE_SLOT, ONE_V0 = 0x1_0000_0007, 4755, 1807, 0xFFFFFF98


def _hybrid_launch(nv, seed, step, B, pairs, num_corr, tr, data_seed):
    g = np.random.default_rng(data_seed)
    pidx = g.integers(0, 5000, B).astype(np.int32)                  # mostly above num_corr: the modulo acts
    r0, r1 = g.integers(100_000, 200_000, B).astype(np.int32), g.integers(200_000, 300_000, B).astype(np.int32)
    (f0, i0), (f1, i1) = buffer((B,), torch.int32), buffer((B,), torch.int32)
    dev = [torch.from_numpy(a).cuda() for a in (pidx, r0, r1)]
    nv.hybrid_assemble(None if pairs is None else torch.from_numpy(pairs).cuda(), *dev, num_corr, tr, rng_state(seed, step),
                       HYBRID_STREAM, i0, i1)
    w0, w1, paired = su.hybrid(seed, step, HYBRID_STREAM, pairs, pidx, r0, r1, num_corr, tr)
    got0, got1 = i0.cpu().numpy(), i1.cpu().numpy()
    assert intact(f0) and intact(f1)
    return got0, got1, w0, w1, paired


@pytest.mark.parametrize('B', [1, 255, 256, 257, 2048])
def test_hybrid_assemble_equals_the_restatement(nv, B):
    """idx0 and idx1 slot for slot against sampler_util.hybrid: true_ratio 0, 0.8 and 1; no pairs (a null table), one pair,
    300 pairs with pair numbers up to 5000."""
    g = np.random.default_rng(B)
    tables = {0: None, 1: g.integers(0, 90_000, (1, 2)).astype(np.int32), 300: g.integers(0, 90_000, (300, 2)).astype(np.int32)}
    for num_corr, pairs in tables.items():
        for tr in (0.0, 0.8, 1.0):
            for step in (3, 2 ** 32 + 5):
                got0, got1, w0, w1, paired = _hybrid_launch(nv, su.SEED, step, B, pairs, num_corr, tr, B + num_corr)
                assert np.array_equal(got0, w0) and np.array_equal(got1, w1), (B, num_corr, tr, step)
                if num_corr == 0 or tr == 0.0:
                    assert not paired.any()
                elif tr == 1.0:
                    assert paired.all() and got0.max() < 100_000
                elif B >= 255:
                    assert 0 < paired.sum() < B


def test_hybrid_assemble_true_ratio_one_pairs_the_draw_that_rounds_to_one(nv):
    """The reference pairs a slot when `np.random.rand() < true_ratio`, so true_ratio = 1 pairs every slot.  The kernel's
    uniform number is float32(v0) * 2^-32, and float32(v0) rounds up to 2^32 for the 128 largest v0: x = 1.0, and `x < 1`
    left that slot unpaired (it did, before hybrid_assemble_kernel was given `|| true_ratio >= 1`).  Pinned on the draw
    (seed 0x1_0000_0007, stream 204, step 4755, slot 1807), v0 = 0xFFFFFF98; every other ratio treats the slot as x = 1.0."""
    assert int(su.rand4(ONE_SEED, ONE_STEP, HYBRID_STREAM, ONE_SLOT)[0]) == ONE_V0 >= 0xFFFFFF80
    assert su.hybrid_x(ONE_SEED, ONE_STEP, HYBRID_STREAM, 2048)[ONE_SLOT] == np.float32(1.0)
    pairs = np.random.default_rng(1).integers(0, 90_000, (300, 2)).astype(np.int32)
    for tr in (1.0, float(np.nextafter(np.float32(1.0), np.float32(0.0))), 0.8):
        got0, got1, w0, w1, paired = _hybrid_launch(nv, ONE_SEED, ONE_STEP, 2048, pairs, 300, tr, 7)
        assert (got0[ONE_SLOT] < 100_000) == (tr == 1.0), tr
        assert np.array_equal(got0, w0) and np.array_equal(got1, w1), tr
        assert paired[ONE_SLOT] == (tr == 1.0) and (tr < 1.0 or paired.all())


# ------------------------------------------------------------------------------------------------
# gather_rows (exact)
# ------------------------------------------------------------------------------------------------
def _gather(nv, src_dev, src_host, idx, dst_offset=0):
    B, d = len(idx), src_host.shape[1]
    full, flat = buffer((B * d + dst_offset,), torch.float32)
    dst = flat[dst_offset:].view(B, d)
    nv.gather_rows(src_dev, torch.tensor(idx, dtype=torch.int32, device='cuda'), dst)
    rows = np.clip(np.asarray(idx, dtype=np.int64), 0, src_host.shape[0] - 1)
    assert torch.equal(dst.cpu(), src_host[rows])
    assert intact(full) and untouched(flat[:dst_offset])


@pytest.mark.parametrize('d', [1, 3, 4, 70])
def test_gather_rows_narrow(nv, d):
    """A 1000-row source, B = 300 with duplicates and B = 1; indices -5 and n_rows + 5 read row 0 and the last row (the
    clamp that the kernel documents)."""
    g = torch.Generator().manual_seed(d)
    src = torch.randn(1000, d, generator=g)
    idx = torch.randint(0, 1000, (300,), generator=g).tolist()
    idx[5], idx[6], idx[7], idx[8], idx[299] = idx[4], -5, 1005, 999, 0
    sd = src.cuda()
    _gather(nv, sd, src, idx)
    _gather(nv, sd, src, [17])
    _gather(nv, sd, src, [-5])
    _gather(nv, sd, src, [1005])


@pytest.mark.parametrize('d', [8200, 8202])
def test_gather_rows_wider_than_the_grid(nv, d):
    """d = 8200: 2050 float4 per row on 2048 threads, the loop's second trip; d = 8202: the scalar loop, five trips."""
    src = torch.randn(5, d, generator=torch.Generator().manual_seed(d))
    sd = src.cuda()
    _gather(nv, sd, src, [4, 0, 2, 2, 4, 1, 3])
    _gather(nv, sd, src, [9, -1, 3])
    _gather(nv, sd, src, [4])


def test_gather_rows_off_16_bytes(nv):
    """A source, then a destination, that starts 4 bytes into its buffer with d = 8: the scalar fallback."""
    g = torch.Generator().manual_seed(3)
    flat = torch.randn(1000 * 8 + 1, generator=g)
    src = flat[1:].view(1000, 8)
    sd = flat.cuda()[1:].view(1000, 8)
    assert sd.data_ptr() % 16 == 4
    idx = torch.randint(0, 1000, (300,), generator=g).tolist()
    _gather(nv, sd, src, idx)
    aligned = src.contiguous()
    _gather(nv, aligned.cuda(), aligned, idx, dst_offset=1)
    _gather(nv, sd, src, idx, dst_offset=3)


# ------------------------------------------------------------------------------------------------
# corr_from_indices (exact)
# ------------------------------------------------------------------------------------------------
def _corr(nv, idx0, idx1):
    B = len(idx0)
    full, corr = buffer((B, B), torch.float32)
    nv.corr_from_indices(torch.from_numpy(idx0).cuda(), torch.from_numpy(idx1).cuda(), corr)
    got = corr.cpu()
    assert torch.equal(got, orc.p_block(None, idx0, idx1))
    assert intact(full)
    return got


@pytest.mark.parametrize('B', [1, 255, 256, 257, 700])
def test_corr_from_indices_with_two_index_lists(nv, B):
    """idx0 != idx1, exact against the oracle's p_block: a value three times in idx1 (1 / 3 in three places of its rows),
    rows of idx0 without a match (all zero), and all of idx1 equal (a row of float32(1 / B))."""
    g = np.random.default_rng(B)
    if B == 1:
        assert float(_corr(nv, np.array([3], dtype=np.int32), np.array([3], dtype=np.int32))[0, 0]) == 1.0
        assert float(_corr(nv, np.array([3], dtype=np.int32), np.array([4], dtype=np.int32))[0, 0]) == 0.0
        return
    idx0, idx1 = g.integers(0, 60, B).astype(np.int32), g.integers(0, 60, B).astype(np.int32)
    three = [0, B // 2, B - 1]
    idx1[three] = 77
    idx0[[1, B - 1]] = 77
    idx0[[2, B - 2]] = 9999
    got = _corr(nv, idx0, idx1)
    third = torch.tensor(1.0) / 3
    for row in (1, B - 1):
        assert torch.equal(got[row].nonzero().flatten(), torch.tensor(three)) and bool((got[row, three] == third).all())
    assert not got[2].any() and not got[B - 2].any()
    same = np.full(B, 5, dtype=np.int32)
    idx0[0], idx0[B - 1] = 5, 5
    got = _corr(nv, idx0, same)
    assert bool((got[0] == torch.tensor(np.float32(1.0) / np.float32(B))).all()) and torch.equal(got[0], got[B - 1])
    assert not got[2].any()


# ------------------------------------------------------------------------------------------------
# csr_block, dense_block, axpby against float64 on the dense matrix
# ------------------------------------------------------------------------------------------------
N0, N1 = 40, 3000
ROW_ONE, ROW_CANCEL, ROW_EMPTY, ROW_LONG = 0, 1, 2, 3
LONG_COLS = np.arange(100, 2100, 2)                       # the 1000 entries of ROW_LONG: first 100, last 2098
CANCEL_COLS, CANCEL_VALS = [11, 12, 13, 14], [0.5, -0.5, 0.25, -0.25]


@functools.lru_cache(maxsize=None)
def block_matrix():
    """A [40, 3000] float32 matrix, dense and as CSR with sorted column indices: a row with a single entry, a row whose four
    entries cancel exactly (dyadic values: in any order of summation), an empty row, a row with 1000 entries on the even
    columns 100..2098, and rows with about 150 positive entries each."""
    g = np.random.default_rng(11)
    M = np.zeros((N0, N1), dtype=np.float32)
    M[ROW_ONE, 5] = 2.5
    M[ROW_CANCEL, CANCEL_COLS] = CANCEL_VALS
    M[ROW_LONG, LONG_COLS] = g.uniform(0.1, 2.0, LONG_COLS.size)
    for r in range(4, N0):
        cols = g.choice(N1, 150, replace=False)
        M[r, cols] = g.uniform(0.1, 2.0, 150)
    indptr, indices, vals = [0], [], []
    for r in range(N0):
        c = np.flatnonzero(M[r])
        indices.append(c)
        vals.append(M[r, c])
        indptr.append(indptr[-1] + c.size)
    csr = (np.asarray(indptr, dtype=np.int32), np.concatenate(indices).astype(np.int32), np.concatenate(vals).astype(np.float32))
    return M, csr


def block_indices(B1, variant=0):
    """idx0: the special rows, duplicates and ordinary rows; idx1: B1 columns whose first entries are the first, an absent and
    the last column of the 1000-entry row and neighbours of the ends (rotated by `variant`, so that B1 = 1 sees each), then
    the four cancelling columns once each, then random columns with duplicates that avoid the cancelling ones."""
    g = np.random.default_rng(B1)
    idx0 = np.array([ROW_LONG, ROW_ONE, ROW_CANCEL, ROW_EMPTY, ROW_LONG, 7, 39, 7, 20, 4, 38, 21], dtype=np.int32)
    special = [100, 101, 2098, 99, 2099, 0, N1 - 1, 5]
    special = special[variant:] + special[:variant] + CANCEL_COLS
    rest = g.integers(20, N1, max(B1 - len(special), 0))
    idx1 = np.concatenate([special, rest])[:B1].astype(np.int32)
    return idx0, idx1


def block_reference(M, idx0, idx1, normalise, w_blk=1.0, add=None, w_add=0.0):
    """(float64 reference, bound on |float32 result - reference|, magnitude |w_blk block| + |w_add add| that the errors are
    reported against) of w_blk * rownorm(M[idx0][:, idx1]) + w_add * add."""
    blk = M.astype(np.float64)[idx0.astype(np.int64)][:, idx1.astype(np.int64)]
    S, A = blk.sum(1), np.abs(blk).sum(1)
    rel = np.zeros(len(idx0))
    if normalise:
        blk = blk / np.where(S == 0, 1.0, S)[:, None]
        rel = su.normalised_row_bound(A, S, len(idx1))
    ref = float(np.float32(w_blk)) * blk
    bound = np.abs(ref) * rel[:, None]                      # the row sum and the quotient
    scale = np.abs(ref)
    if w_blk != 1.0:
        bound += EPS32 * np.abs(ref)                        # the product with w_blk
    if add is not None:
        mix = float(np.float32(w_add)) * add.astype(np.float64)
        bound += EPS32 * np.abs(mix) + EPS32 * (np.abs(ref) + np.abs(mix))        # w_add * add, and the addition
        ref, scale = ref + mix, scale + np.abs(mix)
    return ref, bound, scale


def check_block(got, ref, bound, scale, label):
    err = np.abs(got.astype(np.float64) - ref)
    ulps = float((err[scale > 0] / scale[scale > 0]).max() / EPS32) if (scale > 0).any() else 0.0
    used = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    print(f'ASSEMBLY {label}: largest error {ulps:.2f} u of the magnitude (u = 2^-24), {used:.3f} of the bound')
    assert bool((err <= bound).all()), (label, float((err - bound).max()))
    assert bool((got[ref == 0] == 0).all())


@pytest.mark.parametrize('B1', [1, 256, 257, 600])
def test_csr_block_against_float64(nv, B1):
    """jamie_csr_block on the matrix of block_matrix: raw gathers are exact, normalised rows lie within
    sampler_util.normalised_row_bound of float64; the single-entry row, the cancelling row (sum 0: stays unnormalised), the
    empty row; the first, the last and absent columns of the 1000-entry row (the binary search's ends); row and column
    offsets; an entirely empty matrix.
    Largest error seen on normalised rows, relative to the element: 0 (B1 = 1), 2.14 u (256), 2.25 u (257), 1.98 u (600),
    u = 2^-24: at most 0.009 of the bound, which is the worst case over every order of summation."""
    M, csr = block_matrix()
    dev = [torch.from_numpy(a).cuda() for a in csr]
    for variant in (range(3) if B1 == 1 else (0,)):
        idx0, idx1 = block_indices(B1, variant)
        i0, i1 = torch.from_numpy(idx0).cuda(), torch.from_numpy(idx1).cuda()
        for ro, co in ((0, 0), (1, 2)):
            s0, s1 = np.minimum(idx0, N0 - 1 - ro).astype(np.int32), np.maximum(idx1 - co, 0).astype(np.int32)
            a0, a1 = torch.from_numpy(s0).cuda(), torch.from_numpy(s1).cuda()
            for normalise in (False, True):
                full, out = buffer((len(idx0), B1), torch.float32)
                nv.csr_block(*dev, a0, a1, out, ro, co, normalise)
                ref, bound, scale = block_reference(M, s0 + ro, s1 + co, normalise)
                got = out.cpu().numpy()
                assert intact(full)
                if normalise:
                    check_block(got, ref, bound, scale, f'csr_block B1={B1}')
                else:
                    assert np.array_equal(got, ref.astype(np.float32))
        if B1 >= 256:             # the cancelling row: its columns once each, sum 0, left as it is
            full, out = buffer((len(idx0), B1), torch.float32)
            nv.csr_block(*dev, i0, i1, out, 0, 0, True)
            row = out.cpu().numpy()[2]
            assert np.array_equal(row[8:12], np.float32(CANCEL_VALS)) and not row[12:].any() and not row[:8].any()
    empty = [torch.zeros(N0 + 1, dtype=torch.int32, device='cuda'), torch.zeros(0, dtype=torch.int32, device='cuda'),
             torch.zeros(0, device='cuda')]
    full, out = buffer((len(idx0), B1), torch.float32)
    nv.csr_block(*empty, i0, i1, out, 0, 0, True)
    assert not out.any() and intact(full)


@pytest.mark.parametrize('B1', [1, 256, 257, 600])
def test_dense_block_against_float64(nv, B1):
    """jamie_dense_block on a column slice of a wider matrix (ld = 3010 > N1 = 3000): raw, normalised, and the mix
    0.3 * block + 0.7 * add; zero-sum rows stay unnormalised.
    Largest error seen, u = 2^-24: normalised 0 (B1 = 1), 2.14 u (256), 2.25 u (257), 1.98 u (600) of the element, scaled by
    0.3 up to 2.60 u, at most 0.009 of the bound; mixed 0.86 u (1), 1.25 u (256), 1.36 u (257), 1.50 u (600) of
    |0.3 block| + |0.7 add|, at most 0.68 of the bound (the raw mix: two products and a sum against 2 u)."""
    M, _ = block_matrix()
    wide = np.full((N0, N1 + 10), 1e6, dtype=np.float32)
    wide[:, 7:7 + N1] = M
    Md = torch.from_numpy(wide).cuda()[:, 7:7 + N1]
    assert Md.stride(0) == N1 + 10
    g = np.random.default_rng(B1 + 1)
    for variant in (range(3) if B1 == 1 else (0,)):
        idx0, idx1 = block_indices(B1, variant)
        add = g.standard_normal((len(idx0), B1)).astype(np.float32)
        addd = torch.from_numpy(add).cuda()
        for ro, co in ((0, 0), (1, 2)):
            s0, s1 = np.minimum(idx0, N0 - 1 - ro).astype(np.int32), np.maximum(idx1 - co, 0).astype(np.int32)
            a0, a1 = torch.from_numpy(s0).cuda(), torch.from_numpy(s1).cuda()
            for normalise in (False, True):
                for mixed in (False, True):
                    kw = dict(w_blk=0.3, add=addd, w_add=0.7) if mixed else {}
                    full, out = buffer((len(idx0), B1), torch.float32)
                    nv.dense_block(Md, a0, a1, out, ro, co, normalise, **kw)
                    ref, bound, scale = block_reference(M, s0 + ro, s1 + co, normalise, **({**kw, 'add': add} if mixed else {}))
                    got = out.cpu().numpy()
                    assert intact(full)
                    if normalise or mixed:
                        check_block(got, ref, bound, scale, f'dense_block B1={B1} {"mixed" if mixed else "normalised"}')
                    else:
                        assert np.array_equal(got, ref.astype(np.float32))
    # w_blk alone (add null) scales the block
    full, out = buffer((len(idx0), B1), torch.float32)
    nv.dense_block(Md, a0, a1, out, ro, co, True, w_blk=0.3)
    ref, bound, scale = block_reference(M, s0 + ro, s1 + co, True, w_blk=0.3)
    check_block(out.cpu().numpy(), ref, bound, scale, f'dense_block B1={B1} scaled')
    assert intact(full)


@pytest.mark.parametrize('n', [1, 256, 257, 70_001])
def test_axpby_against_float64(nv, n):
    """out = a x + b y against float64 with a and b as the kernel receives them (float32): two products and a sum, possibly
    contracted, so |error| <= 2 u (|a x| + |b y|); y null: one product, |error| <= u |a x|; out aliasing x."""
    g = torch.Generator().manual_seed(n)
    x, y = torch.randn(n, generator=g), torch.randn(n, generator=g)
    a, b = 0.3, 0.7
    a64, b64 = float(np.float32(a)), float(np.float32(b))
    xd, yd = x.cuda(), y.cuda()
    for with_y in (True, False):
        ref = a64 * x.double() + (b64 * y.double() if with_y else 0)
        bound = (2 if with_y else 1) * EPS32 * ((a64 * x.double()).abs() + (b64 * y.double()).abs() * with_y)
        full, out = buffer((n,), torch.float32)
        nv.axpby(out, a, xd, b, yd if with_y else None)
        assert bool(((out.cpu().double() - ref).abs() <= bound).all()) and intact(full)
        first = out.cpu()
        full, alias = padded(x)
        nv.axpby(alias, a, alias, b, yd if with_y else None)
        assert torch.equal(alias.cpu(), first) and intact(full)
    assert torch.equal(xd.cpu(), x) and torch.equal(yd.cpu(), y)


# ------------------------------------------------------------------------------------------------
# col_stats / standardise
# ------------------------------------------------------------------------------------------------
MEAN_TOL, SD_TOL, CELL_TOL = dict(rtol=1e-12, atol=1e-12), dict(rtol=1e-10, atol=1e-12), dict(rtol=2e-6, atol=1e-6)
CONST_COL, NAN_CELL = 7, (11, 3)


@functools.lru_cache(maxsize=None)
def cells(N, d, f64, const=True, nan=False):
    """[N, d] cells with per-column scale and offset (column 7 constant 3.25 where there is one; `nan`: a NaN at (11, 3)), and
    their float64 statistics and standardised float32 values as numpy's preclass(axis=0) forms them."""
    rng = np.random.default_rng(1000 * N + d)
    X = (rng.standard_normal((N, d)) * rng.uniform(0.1, 30, d) + rng.uniform(-5, 5, d)).astype(np.float64 if f64 else np.float32)
    if const and d > CONST_COL:
        X[:, CONST_COL] = 3.25
    if nan:
        X[NAN_CELL] = np.nan
    X64 = X.astype(np.float64)
    mean, sd = X64.mean(0), X64.std(0)
    with np.errstate(divide='ignore', invalid='ignore'):
        want = (X64 - mean) / sd
    want[np.isnan(want)] = 0
    return X, mean, sd, want.astype(np.float32)


def _standardise(nv, X, R, slice_of_wider):
    """jamie_col_stats + jamie_standardise with explicit ld and n_row_blocks on sentinel-padded buffers."""
    N, d = X.shape
    Xd = torch.from_numpy(X).cuda()
    ld = d
    if slice_of_wider:
        wide = torch.full((N, d + 5), 1e6, dtype=Xd.dtype, device='cuda')
        wide[:, 2:2 + d] = Xd
        Xd, ld = wide[:, 2:2 + d], d + 5
    f64 = int(X.dtype == np.float64)
    (pf, part), (mf, mean), (sf, sd) = buffer((R * d,), torch.float64), buffer((d,), torch.float64), buffer((d,), torch.float64)
    of, out = buffer((N, d), torch.float32)
    nv._call('jamie_col_stats', nv.ptr(Xd), f64, N, d, ld, nv.ptr(part), R, nv.ptr(mean), nv.ptr(sd), nv._stream())
    nv._call('jamie_standardise', nv.ptr(Xd), f64, N, d, ld, nv.ptr(mean), nv.ptr(sd), nv.ptr(out), nv._stream())
    torch.cuda.synchronize()
    assert all(intact(x) for x in (pf, mf, sf, of))
    return mean.cpu().numpy(), sd.cpu().numpy(), out.cpu().numpy()


def _check_standardise(nv, N, d, R, f64, slice_of_wider, const=True, nan=False):
    X, mean, sd, want = cells(N, d, f64, const, nan)
    gm, gs, got = _standardise(nv, X, R, slice_of_wider)
    np.testing.assert_allclose(gm, mean, **MEAN_TOL)
    np.testing.assert_allclose(gs, sd, **SD_TOL)
    np.testing.assert_allclose(got, want, **CELL_TOL)
    assert np.isfinite(got).all()
    if const and d > CONST_COL:
        assert gm[CONST_COL] == 3.25 and gs[CONST_COL] == 0 and not got[:, CONST_COL].any()
    if nan:
        assert np.isnan(gm[NAN_CELL[1]]) and not got[:, NAN_CELL[1]].any()


@pytest.mark.parametrize('R', [1, 3, 1024])
@pytest.mark.parametrize('d', [1, 63, 64, 65, 203])
def test_standardise_against_numpy(nv, d, R):
    """N = 4099 cells, fp32 and fp64, ld = d and a column slice with ld = d + 5, every n_row_blocks: mean, sd and cells at the
    tolerances of test_device_standardisation_matches_numpy; a constant column is 0 everywhere; a NaN cell zeroes its column."""
    for f64 in (False, True):
        for slice_of_wider in (False, True):
            _check_standardise(nv, 4099, d, R, f64, slice_of_wider)
    if d > CONST_COL:
        _check_standardise(nv, 4099, d, R, False, True, nan=True)
        _check_standardise(nv, 4099, d, R, True, False, nan=True)


@pytest.mark.parametrize('N,R', [(1, 1), (1, 8), (3, 8), (3, 1), (2, 1024)])
def test_standardise_with_fewer_rows_than_row_blocks(nv, N, R):
    """N = 1: sd = 0 and every cell is 0 / 0 -> NaN -> 0; N = 3 with 8 row blocks: five blocks have no row."""
    for f64 in (False, True):
        X, mean, sd, want = cells(N, 65, f64, const=False)
        gm, gs, got = _standardise(nv, X, R, slice_of_wider=f64)
        np.testing.assert_allclose(gm, mean, **MEAN_TOL)
        np.testing.assert_allclose(gs, sd, **SD_TOL)
        np.testing.assert_allclose(got, want, **CELL_TOL)
        if N == 1:
            assert not gs.any() and not got.any() and np.array_equal(gm, X[0].astype(np.float64))


@pytest.mark.parametrize('N', [49, 98, 107, 700])
def test_standardise_constant_column_at_any_row_count(nv, N):
    """A constant feature is 0 after standardisation, as in the reference (0 / 0 -> NaN -> 0), whatever N is: the mean must be
    sum / N as numpy forms it.  fl(3.25 N * fl(1 / N)) is one ulp off 3.25 at N = 49, 98, 107 (one N in eight), and the
    feature came out as +-1 when the kernel multiplied by 1 / N."""
    for f64 in (False, True):
        _check_standardise(nv, N, 64, 1, f64, False)
        _check_standardise(nv, N, 64, 3, f64, True)


def test_standardise_refuses_bad_row_block_counts(nv):
    X = torch.randn(100, 8, device='cuda')
    (pf, part), (mf, mean), (sf, sd) = buffer((2048 * 8,), torch.float64), buffer((8,), torch.float64), buffer((8,), torch.float64)
    for R in (0, 1025, -1):
        with pytest.raises(nv.JamieHipError):
            nv._call('jamie_col_stats', nv.ptr(X), 0, 100, 8, 8, nv.ptr(part), R, nv.ptr(mean), nv.ptr(sd), nv._stream())
    with pytest.raises(nv.JamieHipError):                       # ld < d
        nv._call('jamie_col_stats', nv.ptr(X), 0, 100, 8, 7, nv.ptr(part), 4, nv.ptr(mean), nv.ptr(sd), nv._stream())
    torch.cuda.synchronize()
    assert untouched(pf) and untouched(mf) and untouched(sf)

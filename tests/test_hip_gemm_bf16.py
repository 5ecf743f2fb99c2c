"""jamie_gemm_bf16 one launch at a time, in the forms and on the tile configurations the training step launches
(csrc/gemm_bf16.hip; builders and float64 reference in tests/gemm_bf16_util.py, themselves checked by
tests/test_host_gemm_bf16.py).  Run on the MI355X box:  pytest -m gpu tests/test_hip_gemm_bf16.py

Forms: `nt` (forward: bias, split-K slabs), `b_tr` (dX on the weights as stored), `a_tr_b_tr` (dW: partial, store_nt,
accumulate, c_bf16).  Configurations: PRODUCT = 29, 31, 32 (jamie_amd/engine.py), SMALL = -1, 7, 10 (small layers, NT only),
OTHER_V2 = the remaining large-tile ones.  b_tr runs where BN == 128, a_tr where BM == BN == 128 (launch_dma's rules).

Two operand generators.  Integer (A from randint(-4, 5), B = (arange % 13) - 6; {-1, 0, 1} for bf16 outputs): every partial
sum is an integer below 2^24, the product is exact in fp32 in any order, so the device must return the reference itself --
one wrong lane, one lost 8-wide k-chunk, one NaN read from the padding shows at the element it hits.  (For bf16 outputs also
wide integers, B = 16 ((arange % 13) - 6) + 1: still exact in fp32, but nearly every sum has to round, once.)  Random (randn rounded
to bf16) against float64 at test_gemm_bf16's tolerance, rtol 1e-5, atol 1.2e-5 sqrt(K).  C always starts as a sentinel (NaN;
0x7FC1 for bf16) between guard rows: an unwritten element fails the comparison, a write outside the logical block fails
`assert_padding_untouched`.

Shapes (gemm_bf16_util.shapes_for; BM x BN the tile of the configuration):
    (8, 8, 8)                  smallest legal
    (BM + 8, BN + 8, 24)       one partial k-tile only
    (BM + 8, BN + 8, 72)       a full k-tile and an 8-wide tail
    (BM - 8, BN + 8, 200)      three full k-tiles and a tail: more than the 2-buffer ring of 29 holds
    (BM + 8, 8, 72)            narrow N under a wide tile: the clamp min(n0 + lc * 8, N - 8)
    (40, BN + 4, 72)           N % 4 == 0, N % 8 != 0 (NT)
    (BM + 8, BN + 2 | 3, 72)   N % 4 != 0: the scalar epilogue (NT)
    (9 * 128 + 8, 136, 64)     ten M-tiles: the `gi >= ng` branch of the tile order (128-row tiles)
"""
import functools
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_bf16_util as gu  # noqa: E402

pytestmark = pytest.mark.gpu

PRODUCT, SMALL, OTHER_V2, LARGE = gu.PRODUCT, gu.SMALL, gu.OTHER_V2, gu.LARGE
WORST = {'ratio': 0.0, 'partial': 0.0}          # largest error / bound of the random cases, largest per-tile partial error


@pytest.fixture(scope='module')
def nv():
    from jamie_amd import _native
    _native.require_gpu()
    for cfg, tile in gu.TILE.items():          # the shapes below are built from this table
        assert _native.gemm_bf16_tile(512, 512, cfg) == tile, (cfg, tile)
    return _native


def _seed(form, M, N, K):
    return gu.FORMS.index(form) * 1_000_003 + M * 7919 + N * 104_729 + K


@functools.lru_cache(maxsize=None)
def case(form, M, N, K, pads=(0, 0, 0), kind='int', slabs=1, c_bf16=False):
    """Built once per argument set and shared (never written to: launches work on device copies)."""
    return gu.make_case(form, M, N, K, pads=pads, seed=_seed(form, M, N, K), kind=kind, slabs=slabs, c_bf16=c_bf16)


def _dev(c):
    if 'dev' not in c.extra:
        c.extra['dev'] = (c.a_buf.cuda(), c.b_buf.cuda())
    return c.extra['dev']


def problem(nv, c, Cd, **kw):
    A, B = _dev(c)
    return nv.gemm_problem(A, B, Cd[c.c_off:], c.M, c.N, c.K, c.lda, c.ldb, c.ldc, splitk=c.slabs, slab_stride=c.slab_stride,
                           b_tr=c.form != 'nt', a_tr=c.form == 'a_tr_b_tr', c_bf16=c.c_bf16, **kw)


def run(nv, c, cfg, c0=None, **kw):
    """One launch of one problem; the whole C buffer (guards and padding included) back on the host."""
    Cd = (c.c_buf if c0 is None else c0).cuda()
    nv.gemm_bf16([problem(nv, c, Cd, **kw)], cfg)
    torch.cuda.synchronize()
    return Cd.cpu()


def mismatches(c, c_flat, want):
    """Elements of the logical block(s) that differ from `want` ([M, N] or [slabs, M, N], float64 of exact values)."""
    got = c.logical(c_flat)
    want = want.reshape(-1, c.M, c.N)
    want = gu.rne_bf16(want) if c.c_bf16 else want.float()
    assert not c.c_bf16 or got.dtype == torch.bfloat16
    bad = ~(got == want)                        # (a NaN sentinel left behind is a mismatch)
    return int(bad.sum()), (tuple(bad.nonzero()[0].tolist()) if bool(bad.any()) else None)


def check_exact(c, c_flat, want, label):
    n, first = mismatches(c, c_flat, want)
    print(f'{label}: {n} of {c.slabs * c.M * c.N} elements differ' + (f', first at (slab, m, n) = {first}' if n else ''))
    assert n == 0, label
    c.assert_padding_untouched(c_flat)


def check_random(c, c_flat, want, label, tol=None):
    rtol, atol = tol or gu.random_tolerance(c.K)
    err, ratio = gu.error_ratio(c.logical(c_flat).sum(0), want, rtol, atol)
    WORST['ratio'] = max(WORST['ratio'], ratio)
    print(f'{label}: largest error {err:.3e}, {ratio:.3f} of the bound (rtol {rtol:g}, atol {atol:.3e}); worst so far {WORST["ratio"]:.3f}')
    assert ratio <= 1.0, label
    c.assert_padding_untouched(c_flat)


def check_partials(part, want, label, rtol=1e-5, extra=8):
    """Slot by slot; the `extra` slots behind the last tile still NaN; every slot of a tile written (finite)."""
    part = part.cpu().double()
    n = want.numel()
    assert part.numel() == n + extra
    written = bool(torch.isfinite(part[:n]).all())
    rel = float(((part[:n] - want).abs() / want.abs().clamp_min(1e-300)).max()) if written else float('inf')
    WORST['partial'] = max(WORST['partial'], rel if written else 0.0)
    print(f'{label}: {n} tiles, largest per-tile relative error {rel:.3e} (bound {rtol:g}); worst so far {WORST["partial"]:.3e}')
    assert written and rel <= rtol, label
    assert bool(torch.isnan(part[n:]).all()), label + ': a slot beyond the last tile was written'


def nan_partials(n_tiles, extra=8):
    return torch.full((n_tiles + extra,), float('nan'), device='cuda')


def tiles_of(c, cfg):
    bm, bn = gu.TILE[cfg]
    return math.ceil(c.M / bm) * math.ceil(c.N / bn)


FORM_CFG = [(f, c) for f in gu.FORMS for c in gu.legal_cfgs(f, PRODUCT + OTHER_V2 + (SMALL if f == 'nt' else []))]
FORM_PRODUCT = [(f, c) for f in gu.FORMS for c in gu.legal_cfgs(f, PRODUCT)]
FORM_PADDED = [(f, c) for f in gu.FORMS for c in gu.legal_cfgs(f, PRODUCT + (SMALL if f == 'nt' else []))]


def test_parametrisations_are_complete():
    assert len(FORM_CFG) == 15 + 9 + 7 and len(FORM_PRODUCT) == 3 + 3 + 2 and len(FORM_PADDED) == 6 + 3 + 2


# ---- 1. every form on the product's configurations, at the tile edges ---------------------------------------------------
@pytest.mark.parametrize('form,cfg', FORM_CFG)
def test_forms_at_the_tile_edges(nv, form, cfg):
    """form x cfg x shapes_for: the integer case equals the reference element for element, the random case meets float64 at
    rtol 1e-5, atol 1.2e-5 sqrt(K); nothing outside the logical block of C is written."""
    bm, bn = gu.TILE[cfg]
    shapes = gu.shapes_for(bm, bn, form)
    assert len(shapes) == 5 + 3 * (form == 'nt') + (bm == 128)
    for (M, N, K) in shapes:
        c = case(form, M, N, K)
        check_exact(c, run(nv, c, cfg), c.ref, f'{form} cfg {cfg} {(M, N, K)} integer')
        c = case(form, M, N, K, kind='rand')
        check_random(c, run(nv, c, cfg), c.ref, f'{form} cfg {cfg} {(M, N, K)} random')


# ---- 2. padded storage ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('form,cfg', FORM_PADDED)
def test_padded_storage(nv, form, cfg):
    """lda, ldb 8 past the logical width with NaN in the padding and behind the last row; ldc = N + 0, 4, 1 (odd: vec = 0,
    the whole tile through the scalar epilogue) and, at N = BN + 2, + 2 (vec = 1 with a ragged last 4-column piece).  fp32 and,
    on the large tiles, bf16 outputs (pc = 4 keeps their 8-byte alignment, pc = 1 does not).  No NaN reaches an output, no
    padding or guard element of C changes."""
    bm, bn = gu.TILE[cfg]
    shapes = [(bm + 8, bn + 8, 72)] + ([(bm + 8, bn + 2, 72)] if form == 'nt' else [])
    n = 0
    for (M, N, K) in shapes:
        for pc in (0, 4, 1) + ((2,) if N % 4 == 2 else ()):
            c = case(form, M, N, K, pads=(8, 8, pc))
            assert c.lda % 8 == 0 and c.ldb % 8 == 0 and c.ldc == N + pc
            check_exact(c, run(nv, c, cfg), c.ref, f'{form} cfg {cfg} {(M, N, K)} pc {pc} fp32')
            c = case(form, M, N, K, pads=(8, 8, pc), kind='rand')
            check_random(c, run(nv, c, cfg), c.ref, f'{form} cfg {cfg} {(M, N, K)} pc {pc} random')
            if cfg in LARGE:
                c = case(form, M, N, K, pads=(8, 8, pc), kind='int1', c_bf16=True)
                check_exact(c, run(nv, c, cfg), c.ref, f'{form} cfg {cfg} {(M, N, K)} pc {pc} bf16')
            n += 1
    assert n == (7 if form == 'nt' else 3)


# ---- 3. epilogue arms on the product's configurations -----------------------------------------------------------------
def _arm_shapes(form, cfg):
    bm, bn = gu.TILE[cfg]
    return [(bm + 8, bn + 8, 72)] + ([(bm + 8, bn + 2, 72)] if form == 'nt' else [])


@pytest.mark.parametrize('cfg', PRODUCT)
def test_bias_aligned_and_misaligned(nv, cfg):
    """NT with bias: from a 16-byte aligned buffer (float4 loads) and from bias_buf[1:], 4-byte aligned only (vec = 0)."""
    for (M, N, K) in _arm_shapes('nt', cfg):
        c = case('nt', M, N, K)
        g = torch.Generator().manual_seed(N)
        bias_buf = torch.randint(-8, 9, (N + 1,), generator=g).float()
        bd = bias_buf.cuda()
        for off in (0, 1):
            want = c.ref + bias_buf[off:off + N].double()
            check_exact(c, run(nv, c, cfg, bias=bd[off:off + N]), want, f'bias[{off}:] cfg {cfg} {(M, N, K)}')
            assert bd[off:].data_ptr() % 16 == (0 if off == 0 else 4)


@pytest.mark.parametrize('form,cfg', FORM_PRODUCT)
def test_accumulate(nv, form, cfg):
    """C += A B onto an integer C0 (general path: float4 read-modify-write with vec, scalar at N % 4 != 0); with store_nt too."""
    for (M, N, K) in _arm_shapes(form, cfg):
        c = case(form, M, N, K)
        g = torch.Generator().manual_seed(M + N)
        c0 = torch.randint(-16, 17, (M, N), generator=g).float()
        for nt in (False, True):
            out = run(nv, c, cfg, c0=c.with_c0(c0), accumulate=True, store_nt=nt)
            check_exact(c, out, c.ref + c0.double(), f'accumulate {form} cfg {cfg} {(M, N, K)} store_nt {nt}')


@pytest.mark.parametrize('form,cfg', FORM_PRODUCT)
def test_store_nt_changes_no_bit(nv, form, cfg):
    bm, bn = gu.TILE[cfg]
    for (M, N, K) in _arm_shapes(form, cfg) + [(bm, bn, 72)]:
        for kind in ('int', 'rand'):
            c = case(form, M, N, K, kind=kind)
            plain, nt = run(nv, c, cfg), run(nv, c, cfg, store_nt=True)
            same = bool((gu.bits(plain) == gu.bits(nt)).all())
            print(f'store_nt {form} cfg {cfg} {(M, N, K)} {kind}: identical bits {same}')
            assert same
            if kind == 'int':
                check_exact(c, nt, c.ref, f'store_nt {form} cfg {cfg} {(M, N, K)}')
            else:
                check_random(c, nt, c.ref, f'store_nt {form} cfg {cfg} {(M, N, K)} random')


@pytest.mark.parametrize('form,cfg', FORM_PRODUCT)
def test_bf16_output(nv, form, cfg):
    """c_bf16 with and without store_nt: the lean path (N % 4 == 0; an edge tile and an interior one), and for NT the scalar
    path at N = BN + 2 -- with ldc = N (vec = 0: every element through the scalar arm) and ldc = N + 2 (vec = 1: 8-byte stores
    and a scalar last piece).  Operands in {-1, 0, 1}; and the wide integers ('intw'), whose sums are exact in fp32 and DO
    round in bf16: one round-to-nearest-even of the exact value."""
    bm, bn = gu.TILE[cfg]
    todo = [((bm + 8, bn + 8, 72), 0), ((bm, bn, 72), 0), ((bm - 8, bn + 8, 200), 0)]
    if form == 'nt':
        todo += [((bm + 8, bn + 2, 72), 0), ((bm + 8, bn + 2, 72), 2), ((40, bn + 4, 72), 0)]
    rounds = []
    for (M, N, K), pc in todo:
        for kind in ('int1', 'intw'):
            c = case(form, M, N, K, pads=(0, 0, pc), kind=kind, c_bf16=True)
            outs = [run(nv, c, cfg, store_nt=nt) for nt in (False, True)]
            check_exact(c, outs[0], c.ref, f'c_bf16 {form} cfg {cfg} {(M, N, K)} pc {pc} {kind}')
            check_exact(c, outs[1], c.ref, f'c_bf16 + store_nt {form} cfg {cfg} {(M, N, K)} pc {pc} {kind}')
        rounds.append(int((gu.rne_bf16(c.ref).double() != c.ref).sum()))
    print(f'elements of the wide-integer cases that round in bf16, per shape: {rounds}')
    assert min(rounds) > 0


@pytest.mark.parametrize('form,cfg', FORM_PRODUCT)
def test_bf16_output_with_partials_of_the_unrounded_values(nv, form, cfg):
    """c_bf16 + partial (include/jamie_hip.h: `partial` still sums the squares of the fp32 values).  Wide integer operands,
    whose sums round in bf16: the partials of the ROUNDED matrix are off by several times the bound in the small corner tile
    (rounding errors average out over a large one), so partials formed behind the rounding fail here."""
    bm, bn = gu.TILE[cfg]
    todo = [((bm + 8, bn + 8, 72), 0)] + ([((bm + 8, bn + 2, 72), 2)] if form == 'nt' else [])
    for (M, N, K), pc in todo:
        c = case(form, M, N, K, pads=(0, 0, pc), kind='int', c_bf16=True)
        want = gu.tile_partials(c.ref, bm, bn)
        rounded = gu.tile_partials(gu.rne_bf16(c.ref).double(), bm, bn)
        gap = float(((rounded - want).abs() / want).max())
        print(f'partials of the rounded values would be {gap:.2e} off')
        assert gap > 3e-5                  # 3 x the bound of check_partials
        for nt in (False, True):
            part = nan_partials(want.numel())
            out = run(nv, c, cfg, partial=part, store_nt=nt)
            check_exact(c, out, c.ref, f'c_bf16 + partial {form} cfg {cfg} {(M, N, K)} store_nt {nt}')
            check_partials(part, want, f'c_bf16 + partial {form} cfg {cfg} {(M, N, K)} store_nt {nt}')


# ---- 4. per-tile partials ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('form,cfg', [(f, c) for f in gu.FORMS for c in gu.legal_cfgs(f, LARGE)])
def test_plain_store_partials_slot_by_slot(nv, form, cfg):
    """EPI_STORE + partial (large-tile configurations, splitk == 1): slot m_tile + tiles_m * n_tile holds the sum of squares of
    that tile -- edge tiles in M and N, and ten M-tiles x two N-tiles, where the order in which the tiles are computed
    (groups of 8 M-tiles, then the remainder) is not the slot order.  Partials start as NaN: every slot written, none beyond."""
    bm, bn = gu.TILE[cfg]
    for (M, N, K) in [(bm + 8, bn + 8, 72)] + ([(9 * 128 + 8, 136, 64)] if bm == 128 else []):
        for kind in ('int', 'rand'):
            c = case(form, M, N, K, kind=kind)
            want = gu.tile_partials(c.ref, bm, bn)
            assert want.numel() == tiles_of(c, cfg) and len(set(want.tolist())) == want.numel()     # (a swap would show)
            part = nan_partials(want.numel())
            out = run(nv, c, cfg, partial=part)
            (check_exact if kind == 'int' else check_random)(c, out, c.ref, f'partial {form} cfg {cfg} {(M, N, K)} {kind}')
            check_partials(part, want, f'partial {form} cfg {cfg} {(M, N, K)} {kind}')


# ---- 5. EPI_MSE (with its per-tile partials: 4.) --------------------------------------------------------------------------
@pytest.mark.parametrize('cfg', PRODUCT + SMALL)
def test_mse_epilogue(nv, cfg):
    """d = acc + bias - X, C = d * scale, partial[tile] = pscale * sum d^2.  Integer case with scale = 2^-10: `out` exact;
    random case against float64 at test_gemm_bf16_splitk_grouped_mse's tolerances (scale 2 / (M N): rtol 1e-5, atol 1e-7) and,
    tighter, d itself at the plain product's.  X with aux_ld = N (float4 reads where N % 4 == 0) and N + 1 (vec = 0), NaN
    in its padding.  Partials slot by slot at rtol 1e-5, pscale = 2^-7."""
    bm, bn = gu.TILE[cfg]
    shapes = [(100, 152, 80), (bm + 8, bn + 2, 72)] + ([(9 * 128 + 8, 136, 64)] if bm == 128 else [])
    for (M, N, K) in shapes:
        g = torch.Generator().manual_seed(M * N)
        for kind in ('int', 'rand'):
            c = case('nt', M, N, K, kind=kind)
            if kind == 'int':
                bias, X = torch.randint(-8, 9, (N,), generator=g).float(), torch.randint(-8, 9, (M, N), generator=g).float()
                scale, pscale = 2.0 ** -10, 2.0 ** -7
            else:
                bias, X = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
                scale, pscale = 2.0 / (M * N), 2.0 ** -7
            d = c.ref + bias.double() - X.double()
            want_part = gu.tile_partials(d, bm, bn) * pscale
            for pad in (0, 1):
                xbuf, aux_ld = gu.pad_f32(X, pad)
                part = nan_partials(want_part.numel())
                out = run(nv, c, cfg, bias=bias.cuda(), epi=nv.EPI_MSE, aux=(xbuf.cuda(), None, None, None), aux_ld=aux_ld,
                          partial=part, scale=scale, pscale=pscale)
                label = f'MSE cfg {cfg} {(M, N, K)} aux_ld {aux_ld} {kind}'
                if kind == 'int':
                    check_exact(c, out, d * scale, label)
                else:
                    check_random(c, out, d * scale, label, tol=(1e-5, 1e-7))
                    rtol, atol = gu.random_tolerance(K)
                    check_random(c, out, d * scale, label + ' (d at the product tolerance)', tol=(rtol, atol * scale))
                check_partials(part, want_part, label)


# ---- 6. split-K with ragged and empty slices --------------------------------------------------------------------------
@pytest.mark.parametrize('form,cfg', [('nt', c) for c in PRODUCT + SMALL] + [('b_tr', 29)])
def test_split_k_ragged_and_empty_slices(nv, form, cfg):
    """(K, splitk) = (72, 2), (72, 4), (200, 3), (136, 3) at M = BM + 8, N = BN + 8 with bias.  The launcher cuts K into
    kchunk = ceil(ceil(K / splitk) / 64) * 64: 64, 64, 128, 64 -- so the slabs cover k in
        (72, 2):  [0, 64) [64, 72)
        (72, 4):  [0, 64) [64, 72) and slabs 2, 3 EMPTY (kbeg = 128, 192 >= K)
        (200, 3): [0, 128) [128, 200) and slab 2 EMPTY (kbeg = 256 >= K)
        (136, 3): [0, 64) [64, 128) [128, 136)
    (gemm_bf16_util.k_slices, checked against these in tests/test_host_gemm_bf16.py).  Every slab is the product over its own
    slice, slab 0 alone carries the bias, an empty slab is zero everywhere (no sentinel left); the gaps between slabs keep
    their sentinels."""
    bm, bn = gu.TILE[cfg]
    M, N = bm + 8, bn + 8
    g = torch.Generator().manual_seed(cfg + 50)
    bias = torch.randint(-8, 9, (N,), generator=g).float()
    bd = bias.cuda()
    for K, sk in gu.SPLITK:
        slices = gu.k_slices(K, sk)
        empty = [s for s, (k0, k1) in enumerate(slices) if k0 >= k1]
        assert empty == {(72, 2): [], (72, 4): [2, 3], (200, 3): [2], (136, 3): []}[(K, sk)]
        c = case(form, M, N, K, slabs=sk)
        out = run(nv, c, cfg, bias=bd)
        want = torch.stack([c.product(k0, k1) + (bias.double() if s == 0 else 0) for s, (k0, k1) in enumerate(slices)])
        check_exact(c, out, want, f'split-K {form} cfg {cfg} K {K} / {sk} slab by slab')
        got = c.logical(out)
        for s in empty:
            nz = int((gu.bits(got[s]) << 1 != 0).sum())          # +-0 only
            print(f'  slab {s} (empty slice): {nz} non-zero elements')
            assert nz == 0 and float(want[s].abs().max()) == 0.0
        assert torch.equal(got.double().sum(0), c.ref + bias.double())
        c = case(form, M, N, K, kind='rand', slabs=sk)
        check_random(c, run(nv, c, cfg, bias=bd), c.ref + bias.double(), f'split-K {form} cfg {cfg} K {K} / {sk} random, slabs summed')


# ---- 7. a full group -----------------------------------------------------------------------------------------------------
def _run_group(nv, group, cfg, label):
    bm, bn = gu.TILE[cfg]
    assert gu.group_tiles(group, bm, bn) == gu.GROUP_COUNTS and len(group) == nv.MAX_GEMM_GROUP
    todo, probs = [], []
    for i, (form, M, N, K, sk, _) in enumerate(group):
        dw = form == 'a_tr_b_tr'
        c = case(form, M, N, K, pads=(8, 8, 0), kind='int1' if dw else 'int', slabs=sk, c_bf16=dw)
        Cd = c.c_buf.cuda()
        kw, part, bias = {}, None, None
        if dw:
            part = nan_partials(tiles_of(c, cfg))
            kw = dict(partial=part, store_nt=True)
        elif form == 'nt' and i % 2:
            bias = torch.randint(-8, 9, (N,), generator=torch.Generator().manual_seed(i)).float()
            kw = dict(bias=bias.cuda())
        probs.append(problem(nv, c, Cd, **kw))
        todo.append((c, Cd, part, bias))
    nv.gemm_bf16(probs, cfg)
    torch.cuda.synchronize()
    for i, (c, Cd, part, bias) in enumerate(todo):
        want = torch.stack([c.product(k0, k1) for k0, k1 in gu.k_slices(c.K, c.slabs)])
        if bias is not None:
            want = want + bias.double()
        check_exact(c, Cd.cpu(), want, f'{label} problem {i} {c.form} {(c.M, c.N, c.K)} x {c.slabs}')
        if part is not None:
            check_partials(part, gu.tile_partials(c.ref, bm, bn), f'{label} problem {i} partials')


def test_full_group_as_the_backward_launch_mixes_it(nv):
    """Eight problems in one launch on 29 -- dX (b_tr, splitk 2), dW (a_tr + b_tr with partial, store_nt, c_bf16), one plain
    NT -- with 1, 3, 5, 2, 7, 9, 11 and 4 tiles: no prefix of the list is a multiple of 8 tiles, so every problem starts on
    a rotated XCD and every remainder term of the problem decode is live; one dW has 11 M-tiles (tile-order remainder
    inside a group).  Every output exact, every element written, no guard touched, every partial slot written."""
    _run_group(nv, gu.mixed_group(), 29, 'mixed group cfg 29')


@pytest.mark.parametrize('cfg', [31, 32])
def test_full_group_of_forward_products(nv, cfg):
    """Eight NT problems with the same tile counts, every N % 4, bias on every second one."""
    _run_group(nv, gu.nt_group(*gu.TILE[cfg]), cfg, f'NT group cfg {cfg}')


# ---- 8. output beyond 4 GiB ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cfg', [29, 31])
def test_output_beyond_4gib(nv, cfg):
    """C of 33004 x 33004 fp32 (4.36 GB): c_ext >= 0xFFFFFFF0 sends a plain, vector-aligned store down the general path with
    its 64-bit addresses (the lean path's buffer descriptor cannot span it).  Every element written (C starts as NaN, checked
    on the device); sampled rows and columns, those either side of byte offset 2^32 and the last tile row and column among
    them, exact on integer operands.  The one large case of this file: the path cannot be reached below 4 GiB."""
    M = N = 33004
    K = 64
    assert ((M - 1) * N + N) * 4 >= 0xFFFFFFF0 and N % 4 == 0
    g = torch.Generator().manual_seed(cfg)
    a = torch.randint(-4, 5, (M, K), generator=g).float()
    b = (torch.arange(N * K, dtype=torch.float32).reshape(N, K) % 13) - 6
    out = torch.full((M, N), float('nan'), device='cuda')
    nv.gemm_bf16([nv.gemm_problem(a.to(torch.bfloat16).cuda(), b.to(torch.bfloat16).cuda(), out, M, N, K, K, K, N)], cfg)
    finite = bool(torch.isfinite(out).all())
    print(f'cfg {cfg}: all of C finite: {finite}')
    assert finite
    edge = (1 << 32) // (4 * N)
    rows = torch.tensor(sorted({0, 127, 128, edge - 1, edge, edge + 1, 32767, 32768, 32895, 32896, N - 1}
                               | set(torch.randint(0, M, (8,), generator=g).tolist())))
    cols = torch.tensor(sorted({0, 127, 128, 32767, 32768, 32895, 32896, N - 1} | set(torch.randint(0, N, (8,), generator=g).tolist())))
    bad_r = int((out[rows.cuda()].cpu() != a[rows] @ b.t()).sum())
    bad_c = int((out[:, cols.cuda()].cpu() != a @ b[cols].t()).sum())
    print(f'cfg {cfg}: {bad_r} wrong elements in {rows.numel()} rows, {bad_c} in {cols.numel()} columns')
    del out
    torch.cuda.empty_cache()
    assert bad_r == 0 and bad_c == 0


# ---- 9. repeatability ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('form', gu.FORMS)
def test_two_launches_give_identical_bits(nv, form):
    c = case(form, 136, 136, 200, kind='rand')
    kw = dict(partial=nan_partials(4)) if form == 'a_tr_b_tr' else {}
    first = run(nv, c, 29, **kw)
    p1 = kw['partial'].clone() if kw else None
    second = run(nv, c, 29, **kw)
    same = bool((gu.bits(first) == gu.bits(second)).all())
    print(f'{form}: identical bits {same}')
    assert same
    if kw:
        assert bool((gu.bits(p1.cpu()) == gu.bits(kw['partial'].cpu())).all())


# ---- what the launcher refuses ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('form,cfg,kw', [('nt', 35, {}), ('b_tr', 26, {}), ('b_tr', 7, {}), ('a_tr_b_tr', 31, {}),
                                          ('a_tr_b_tr', 10, {}), ('nt', 10, dict(partial=True)), ('nt', 7, dict(c_bf16=True)),
                                          ('nt', 29, dict(partial=True, slabs=2))])
def test_illegal_configurations_raise_and_write_nothing(nv, form, cfg, kw):
    """b_tr outside the 128-column large tiles, a_tr outside the 128 x 128 ones, an unknown configuration, plain-store partials
    or bf16 output on a small tile, partials with split-K: JamieHipError, and C keeps every sentinel."""
    kw = dict(kw)
    c = case(form, 136, 136, 72, slabs=kw.pop('slabs', 1), kind='int1' if kw.get('c_bf16') else 'int',
             c_bf16=bool(kw.pop('c_bf16', False)))
    if kw.pop('partial', False):
        kw['partial'] = nan_partials(8)
    Cd = c.c_buf.cuda()
    with pytest.raises(nv.JamieHipError):
        nv.gemm_bf16([problem(nv, c, Cd, **kw)], cfg)
    torch.cuda.synchronize()
    assert bool((gu.bits(Cd.cpu()) == gu.bits(c.c_buf)).all())
    if 'partial' in kw:
        assert bool(torch.isnan(kw['partial']).all())

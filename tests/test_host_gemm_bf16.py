"""What the bf16 GEMM device tests (tests/test_hip_gemm_bf16.py) rest on, checked on the CPU with the reference alone
(tests/gemm_bf16_util.py): the integer cases are exact in fp32 whatever the order of summation, the padded builders put
NaN where they say and nowhere else, the per-tile partials sit in the documented slots, every shape is one the launcher
accepts, and no parametrisation is empty."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_bf16_util as gu  # noqa: E402

ALL_CFGS = gu.PRODUCT + gu.OTHER_V2 + gu.SMALL


def _all_integer_cases():
    """(form, M, N, K) of every integer case of the device file: the shape table on every tile, the split-K, MSE, group and
    4 GiB shapes."""
    seen = set()
    for cfg in ALL_CFGS:
        bm, bn = gu.TILE[cfg]
        for form in gu.FORMS:
            if not gu.legal(form, cfg):
                continue
            for s in gu.shapes_for(bm, bn, form):
                seen.add((form,) + s)
            for K, _ in gu.SPLITK:
                seen.add((form, bm + 8, bn + 8, K))
        seen.add(('nt', 100, 152, 80))
        for (form, M, N, K, _, _) in gu.nt_group(bm, bn):
            seen.add((form, M, N, K))
    for (form, M, N, K, _, _) in gu.mixed_group():
        seen.add((form, M, N, K))
    return sorted(seen)


def test_integer_cases_are_exact_in_fp32():
    """max |ref| < 2^24 -- and so is the sum of the absolute values of the terms of every element, hence every partial sum
    in any order -- for each integer case; with the accumulate start C0 (|C0| <= 16) and the bias (|bias| <= 8) on top."""
    cases = _all_integer_cases()
    assert len(cases) >= 60
    worst = 0.0
    for (form, M, N, K) in cases:
        c = gu.make_case(form, M, N, K, kind='int', seed=1)
        absum = gu.form_product(form, c.a.abs(), c.b.abs(), 0, K)
        assert float(c.ref.abs().max()) <= float(absum.max())
        worst = max(worst, float(absum.max()) + 16 + 8)
        assert torch.equal(c.ref.float().double(), c.ref)
    print(f'largest sum of |terms| + |C0| + |bias| over {len(cases)} integer cases: {worst:.0f} (2^24 = {2 ** 24})')
    assert worst < 2 ** 24
    # the 4 GiB case: K = 64, |a| <= 4, |b| <= 6
    assert 64 * 4 * 6 < 2 ** 24


def test_bf16_output_cases_round_an_exact_fp32_once():
    """c_bf16 cases: operands in {-1, 0, 1}, |ref| <= K; the expected tensor is the RNE rounding of an exactly representable
    fp32, and -- |ref| <= 256 = 2^8 -- even exact in bf16 (8 significant bits), so a double rounding could not hide either."""
    n = 0
    for (form, M, N, K) in _all_integer_cases():
        if K > 256 or M * N > 400_000:
            continue
        c = gu.make_case(form, M, N, K, kind='int1', seed=2, c_bf16=True)
        assert float(c.ref.abs().max()) <= K
        want = gu.rne_bf16(c.ref)
        assert torch.equal(want.double(), c.ref)
        assert c.c_buf.dtype == torch.bfloat16 and bool((gu.bits(c.c_buf) == gu.BF16_SENTINEL).all())
        n += 1
    assert n >= 60
    # the wide integers (bf16 outputs that must round): operands exact in bf16, sums of |terms| below 2^24, most sums round
    for form in gu.FORMS:
        for (M, N, K) in ((136, 136, 72), (120, 136, 200)):
            c = gu.make_case(form, M, N, K, kind='intw', seed=2, c_bf16=True)
            assert float(c.b.float().abs().max()) == 97 and torch.equal(c.b.float() % 2, torch.ones(c.b.shape))
            assert float(gu.form_product(form, c.a.abs(), c.b.abs(), 0, K).max()) < 2 ** 24
            assert float((gu.rne_bf16(c.ref).double() != c.ref).double().mean()) > 0.5
    # rne_bf16 rounds to nearest even where it has to: 257 -> 256, 259 -> 260, 258 stays
    assert gu.rne_bf16(torch.tensor([257., 258., 259., -257.], dtype=torch.float64)).tolist() == [256., 258., 260., -256.]
    with pytest.raises(AssertionError):
        gu.rne_bf16(torch.tensor([2.0 ** 24 + 1], dtype=torch.float64))


def test_integer_mse_epilogue_is_exact():
    """(acc + bias - X) * scale with integer-valued bias and X, scale = 2^-10: the difference is an integer below 2^24 and the
    product a power-of-two scaling far above the subnormals, so `out` has one right answer in fp32."""
    scale = 2.0 ** -10
    for cfg in gu.PRODUCT + gu.SMALL:
        bm, bn = gu.TILE[cfg]
        for (M, N, K) in ((100, 152, 80), (bm + 8, bn + 2, 72)):
            c = gu.make_case('nt', M, N, K, kind='int', seed=3)
            g = torch.Generator().manual_seed(5)
            bias = torch.randint(-8, 9, (N,), generator=g).double()
            X = torch.randint(-8, 9, (M, N), generator=g).double()
            d = c.ref + bias - X
            assert float(d.abs().max()) < 2 ** 24 and torch.equal(d, d.round())
            out = d * scale
            assert torch.equal(out.float().double(), out)
            nz = out[out != 0].abs()
            assert float(nz.min()) >= scale > 2.0 ** -126


@pytest.mark.parametrize('form', gu.FORMS)
@pytest.mark.parametrize('pads', [(0, 0, 0), (8, 8, 0), (8, 8, 4), (8, 8, 1), (16, 24, 2)])
def test_padded_builders_put_nan_on_padding_only(form, pads):
    M, N, K = 136, 130 if form == 'nt' else 136, 72
    for slabs, bf in ((1, False), (3, False), (1, True)):
        c = gu.make_case(form, M, N, K, pads=pads, kind='rand', seed=7, slabs=slabs, c_bf16=bf)
        plain = gu.make_case(form, M, N, K, kind='rand', seed=7, slabs=slabs, c_bf16=bf)
        assert torch.equal(c.ref, plain.ref) and torch.equal(c.a, plain.a) and torch.equal(c.b, plain.b)
        for buf, ld, t, pad in ((c.a_buf, c.lda, c.a, pads[0]), (c.b_buf, c.ldb, c.b, pads[1])):
            rows, cols = t.shape
            assert ld == cols + pad and ld % 8 == 0 and buf.numel() == rows * ld + gu.GUARD and gu.GUARD >= 64
            img = buf[:rows * ld].view(rows, ld)
            assert torch.equal(img[:, :cols], t) and bool(torch.isfinite(t.float()).all())
            assert bool(torch.isnan(img[:, cols:].float()).all()) and bool(torch.isnan(buf[rows * ld:].float()).all())
        # C: sentinel everywhere, one guard row on each side, slabs a multiple of 4 apart and at least M * ldc
        assert c.ldc == N + pads[2] and c.c_off == c.ldc
        assert c.slab_stride % 4 == 0 and c.slab_stride >= M * c.ldc + gu.SLAB_GAP
        assert c.c_buf.numel() == 2 * c.ldc + slabs * c.slab_stride
        if bf:
            assert bool((gu.bits(c.c_buf) == gu.BF16_SENTINEL).all())
        assert bool(torch.isnan(c.c_buf.float()).all())
        mask = c.logical_mask()
        assert int(mask.sum()) == slabs * M * N and not bool(mask[:c.c_off].any()) and not bool(mask[-c.ldc:].any())
        c.assert_padding_untouched(c.c_buf.clone())
        # the helper sees a write to any kind of padding: row padding, the gap between slabs, either guard row
        spots = [0, c.c_off - 1, c.c_buf.numel() - 1, c.c_off + (slabs - 1) * c.slab_stride + M * c.ldc]
        if pads[2]:
            spots.append(c.c_off + N)
        for pos in spots:
            dirty = c.c_buf.clone()
            dirty[pos] = 1.0
            with pytest.raises(AssertionError):
                c.assert_padding_untouched(dirty)
        # ... a NaN with another payload too, and a write inside the logical block is none of its business
        dirty = c.c_buf.clone()
        gu.bits(dirty)[0] += 1
        with pytest.raises(AssertionError):
            c.assert_padding_untouched(dirty)
        filled = c.c_buf.clone()
        filled[mask] = 3.0
        c.assert_padding_untouched(filled)
        assert torch.equal(c.logical(filled), torch.full((slabs, M, N), 3.0, dtype=filled.dtype))
        if slabs == 1:
            c0 = torch.arange(M * N, dtype=torch.float32).reshape(M, N) % 7
            assert torch.equal(c.logical(c.with_c0(c0))[0].float(), c0)
            c.assert_padding_untouched(c.with_c0(c0))


def test_product_slices_add_up_and_follow_the_form():
    for form in gu.FORMS:
        c = gu.make_case(form, 16, 24, 200, kind='int', seed=9)
        a, b = c.a.double(), c.b.double()
        want = {'nt': lambda: a @ b.t(), 'b_tr': lambda: a @ b, 'a_tr_b_tr': lambda: a.t() @ b}[form]()
        assert torch.equal(c.ref, want) and c.ref.shape == (16, 24)
        for K, sk in gu.SPLITK:
            cc = gu.make_case(form, 16, 24, K, kind='int', seed=9)
            parts = [cc.product(k0, k1) for k0, k1 in gu.k_slices(K, sk)]
            assert torch.equal(sum(parts), cc.ref)


def test_split_k_slices_are_the_launchers():
    """kchunk = ceil(ceil(K / splitk) / 64) * 64; (72, 4) leaves slabs 2 and 3 empty, (200, 3) slab 2; the other two none."""
    assert [gu.kchunk(K, s) for K, s in gu.SPLITK] == [64, 64, 128, 64]
    assert gu.k_slices(72, 2) == [(0, 64), (64, 72)]
    assert gu.k_slices(72, 4) == [(0, 64), (64, 72), (128, 72), (192, 72)]
    assert gu.k_slices(200, 3) == [(0, 128), (128, 200), (256, 200)]
    assert gu.k_slices(136, 3) == [(0, 64), (64, 128), (128, 136)]
    empty = {(K, s): [i for i, (k0, k1) in enumerate(gu.k_slices(K, s)) if k0 >= k1] for K, s in gu.SPLITK}
    assert empty == {(72, 2): [], (72, 4): [2, 3], (200, 3): [2], (136, 3): []}


def test_tile_partials_slot_order():
    """2 x 3 tiles by hand: tile (i, j) holds the value 1 + i + 2 j everywhere, so its sum of squares names it; slot = i + 2 j."""
    BM, BN = 4, 8
    M, N = 6, 19                                     # ragged last tile in both directions
    x = torch.zeros(M, N, dtype=torch.float64)
    for i in range(2):
        for j in range(3):
            x[i * BM:(i + 1) * BM, j * BN:(j + 1) * BN] = 1 + i + 2 * j
    got = gu.tile_partials(x, BM, BN)
    rows, cols = [4, 2], [8, 8, 3]
    want = [rows[i] * cols[j] * (1 + i + 2 * j) ** 2 for j in range(3) for i in range(2)]
    assert got.tolist() == [float(w) for w in want]
    assert got[1 + 2 * 2] == 2 * 3 * 36 and got[0 + 2 * 1] == 4 * 8 * 9
    g = torch.Generator().manual_seed(1)
    y = torch.randn(1160, 136, generator=g).double()
    p = gu.tile_partials(y, 128, 128)
    assert p.numel() == 20 and abs(float(p.sum()) - float((y ** 2).sum())) <= 1e-12 * float((y ** 2).sum())


def test_shapes_satisfy_the_launchers_argument_rules():
    """K, lda, ldb multiples of 8 (with the paddings the device tests use), M % 8 for a_tr, N % 8 for b_tr; every row of the
    table present; the piece of code each row is there for is the one it reaches."""
    n = 0
    for cfg in ALL_CFGS:
        bm, bn = gu.TILE[cfg]
        for form in gu.FORMS:
            if not gu.legal(form, cfg):
                continue
            shapes = gu.shapes_for(bm, bn, form)
            assert len(shapes) == 5 + (3 if form == 'nt' else 0) + (1 if bm == 128 else 0)
            assert len(set(shapes)) == len(shapes)
            for (M, N, K) in shapes:
                for pa, pb in ((0, 0), (8, 8)):
                    c_lda = (M if form == 'a_tr_b_tr' else K) + pa
                    c_ldb = (K if form == 'nt' else N) + pb
                    assert K % 8 == 0 and K >= 8 and c_lda % 8 == 0 and c_ldb % 8 == 0
                assert form != 'a_tr_b_tr' or (M % 8 == 0 and M >= 8)
                assert form == 'nt' or (N % 8 == 0 and N >= 8)
                assert K <= 200
                n += 1
            assert shapes[0] == (8, 8, 8)
            assert shapes[1][2] < gu.BK and shapes[2][2] == gu.BK + 8 and shapes[3][2] == 3 * gu.BK + 8
            assert shapes[3][0] < bm < shapes[2][0] and shapes[2][1] > bn and shapes[4][1] == 8
            if form == 'nt':
                assert [s[1] % 4 for s in shapes[5:8]] == [0, 2, 3] and shapes[5][1] % 8 == 4
            if bm == 128:
                tm = math.ceil(shapes[-1][0] / bm)
                assert tm > 8 and tm % 8 != 0
                assert math.ceil(shapes[-1][1] / bn) == (2 if bn == 128 else 1)
    # nt: 15 configurations x 8 rows + 8 with 128-row tiles; b_tr: 9 x 5 + 7; a_tr + b_tr: 7 x 5 + 7
    assert n == 128 + 52 + 42, n


def test_legal_configurations_per_form():
    assert gu.legal_cfgs('nt', ALL_CFGS) == ALL_CFGS
    assert gu.legal_cfgs('b_tr', ALL_CFGS) == [29, 31, 32, 23, 24, 25, 30, 33, 34]
    assert gu.legal_cfgs('a_tr_b_tr', ALL_CFGS) == [29, 32, 24, 25, 30, 33, 34]
    assert gu.PRODUCT == [29, 31, 32] and gu.SMALL == [-1, 7, 10] and gu.OTHER_V2 == [23, 24, 25, 26, 27, 28, 30, 33, 34]
    assert set(gu.TILE) == set(ALL_CFGS)


def test_groups_have_the_tile_counts_and_no_aligned_prefix():
    assert sorted(gu.GROUP_COUNTS) == sorted([1, 3, 5, 7, 2, 9, 11, 4]) and len(gu.GROUP_COUNTS) == 8
    pre = [sum(gu.GROUP_COUNTS[:i]) for i in range(1, 8)]
    assert all(p % 8 for p in pre), pre
    mixed = gu.mixed_group()
    assert gu.group_tiles(mixed, 128, 128) == gu.GROUP_COUNTS
    assert sorted(f for f, *_ in mixed) == ['a_tr_b_tr'] * 5 + ['b_tr'] * 2 + ['nt']
    for (form, M, N, K, sk, (tm, tn)) in mixed:
        assert (math.ceil(M / 128), math.ceil(N / 128)) == (tm, tn)
        assert K % 8 == 0 and (form != 'a_tr_b_tr' or M % 8 == 0) and (form == 'nt' or N % 8 == 0)
        assert (sk == 2) == (form == 'b_tr')
    assert any(tm > 8 and tm % 8 for *_, (tm, tn) in mixed)         # the remainder branch of the tile order, inside a group
    for cfg in (31, 32):
        bm, bn = gu.TILE[cfg]
        grp = gu.nt_group(bm, bn)
        assert gu.group_tiles(grp, bm, bn) == gu.GROUP_COUNTS
        assert all(K % 8 == 0 for (_, _, _, K, _, _) in grp)
        assert {N % 4 for (_, _, N, _, _, _) in grp} == {0, 1, 2, 3}

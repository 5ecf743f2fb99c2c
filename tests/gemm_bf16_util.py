"""Host side of the bf16 GEMM tests (tests/test_hip_gemm_bf16.py; held to its own claims by tests/test_host_gemm_bf16.py):
case builders in padded storage, the float64 reference, per-tile sums of squares in the documented slot order and the
smallest shapes at which each piece of `gemm_bf16_dma2_body` / `gemm_bf16_dma_kernel` (csrc/gemm_bf16.hip) runs.  Pure
torch / numpy on the CPU: nothing here loads the library.

Forms, as `jamie_gemm_bf16` takes them (include/jamie_hip.h):
    nt          A [M, K] (lda >= K), B [N, K] (ldb >= K)                       forward
    b_tr        A [M, K] (lda >= K), B [K, N] (ldb >= N), N % 8 == 0           dX on the weights as stored
    a_tr_b_tr   A [K, M] (lda >= M), B [K, N] (ldb >= N), M % 8 == N % 8 == 0  dW on dy and a as the layers wrote them
"""
import math
from dataclasses import dataclass, field

import numpy as np
import torch

FORMS = ('nt', 'b_tr', 'a_tr_b_tr')

# the tile configurations the tests launch
PRODUCT = [29, 31, 32]                                   # jamie_amd/engine.py: BF16_CFG_DW, BF16_CFG_ROWS_WIDE, BF16_CFG_ROWS
SMALL = [-1, 7, 10]                                      # small layers: the library default resolves to 7 or 10 (NT form only)
OTHER_V2 = [23, 24, 25, 26, 27, 28, 30, 33, 34]          # the other large-tile (LDS-DMA, second kernel) configurations
# block tile of each of them (the switch of gemm_bf16_impl); the device tests hold nv.gemm_bf16_tile to this table
TILE = {-1: (64, 64), 7: (64, 64), 10: (64, 64), 23: (256, 128), 24: (128, 128), 25: (128, 128), 26: (128, 256),
        27: (64, 64), 28: (256, 256), 29: (128, 128), 30: (128, 128), 31: (256, 128), 32: (128, 128), 33: (128, 128),
        34: (128, 128)}
LARGE = PRODUCT + OTHER_V2

BF16_SENTINEL = 0x7FC1                                   # a quiet NaN no rounding produces from finite data
GUARD = 64                                               # NaN elements behind the last row of an operand
SLAB_GAP = 8                                             # sentinel elements between two split-K slabs (keeps slab_stride % 4 == 0)
BK = 64                                                  # k-tile of every LDS-DMA configuration


def legal(form, cfg):
    """launch_dma's own rules: b_tr needs a large-tile configuration with BN == 128, a_tr one with BM == BN == 128."""
    bm, bn = TILE[cfg]
    if form == 'nt':
        return True
    if cfg not in LARGE:
        return False
    return bn == 128 if form == 'b_tr' else (bm == 128 and bn == 128)


def legal_cfgs(form, cfgs):
    return [c for c in cfgs if legal(form, c)]


def shapes_for(BM, BN, form):
    """One (M, N, K) per row of the table in the module docstring of tests/test_hip_gemm_bf16.py: the smallest shape at
    which that piece of code runs.  a_tr needs M % 8 == 0, b_tr N % 8 == 0; the N % 8 != 0 rows are NT only; the tile-order
    remainder branch (tiles_m > 8, tiles_m % 8 != 0) exists in the large-tile kernel and is taken with 128-row tiles."""
    s = [(8, 8, 8),                                      # smallest legal
         (BM + 8, BN + 8, 24),                           # one partial k-tile only
         (BM + 8, BN + 8, 72),                           # full tile + 8-wide tail
         (BM - 8, BN + 8, 200),                          # three full tiles + tail: more k-tiles than a 2-buffer ring
         (BM + 8, 8, 72)]                                # narrow N under a wide tile: min(n0 + lc * 8, N - 8) clamps
    if form == 'nt':
        s += [(40, BN + 4, 72),                          # N % 4 == 0, N % 8 != 0
              (BM + 8, BN + 2, 72),                      # N % 4 != 0: scalar epilogue
              (BM + 8, BN + 3, 72)]
    if BM == 128:
        s += [(9 * 128 + 8, 136, 64)]                    # ten M-tiles: one full group of 8 and a remainder of 2
    return s


SPLITK = [(72, 2), (72, 4), (200, 3), (136, 3)]


def kchunk(K, splitk):
    """K slice of one split-K slab, as launch_dma forms it."""
    return -(-(-(-K // splitk)) // BK) * BK


def k_slices(K, splitk):
    """[(kbeg, kend)] per slab; kbeg >= kend is an empty slice (the slab is all zeros)."""
    kc = kchunk(K, splitk)
    return [(s * kc, min(K, (s + 1) * kc)) for s in range(splitk)]


def bf16_nan(n):
    return torch.full((n,), float('nan'), dtype=torch.bfloat16)


def _stored_shapes(form, M, N, K):
    a = (K, M) if form == 'a_tr_b_tr' else (M, K)
    b = (N, K) if form == 'nt' else (K, N)
    return a, b


def pad_operand(t, pad):
    """[rows, cols] -> flat bf16 buffer of rows * (cols + pad) + GUARD elements, NaN wherever `t` is not; the leading dimension."""
    rows, cols = t.shape
    ld = cols + pad
    buf = bf16_nan(rows * ld + GUARD)
    buf[:rows * ld].view(rows, ld)[:, :cols] = t.to(torch.bfloat16)
    return buf, ld


def pad_f32(t, pad):
    """The fp32 twin (the X of the MSE epilogue)."""
    rows, cols = t.shape
    ld = cols + pad
    buf = torch.full((rows * ld + GUARD,), float('nan'))
    buf[:rows * ld].view(rows, ld)[:, :cols] = t
    return buf, ld


def bits(t):
    """Bit pattern view of an fp32 / bf16 tensor (NaN sentinels compare equal to themselves here)."""
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def form_product(form, a, b, k0, k1):
    """float64 product of the stored operands over k in [k0, k1)."""
    a, b = a.double(), b.double()
    if form == 'nt':
        return a[:, k0:k1] @ b[:, k0:k1].t()
    if form == 'b_tr':
        return a[:, k0:k1] @ b[k0:k1]
    return a[k0:k1].t() @ b[k0:k1]


@dataclass
class Case:
    form: str
    M: int
    N: int
    K: int
    kind: str                     # 'int' | 'int1' (c_bf16: -1, 0, 1) | 'rand'
    a: torch.Tensor               # logical operands as stored, bf16
    b: torch.Tensor
    a_buf: torch.Tensor           # padded storage, flat
    b_buf: torch.Tensor
    lda: int
    ldb: int
    ldc: int
    c_buf: torch.Tensor           # flat, sentinel everywhere: guard row | slabs | guard row
    c_off: int                    # element offset of C inside c_buf (= ldc: one guard row in front)
    slabs: int
    slab_stride: int
    ref: torch.Tensor             # float64 [M, N]
    extra: dict = field(default_factory=dict)

    @property
    def c_bf16(self):
        return self.c_buf.dtype == torch.bfloat16

    def product(self, k0=0, k1=None):
        """float64 product over k in [k0, k1) (a split-K slab's share)."""
        k1 = self.K if k1 is None else k1
        if k1 <= k0:
            return torch.zeros(self.M, self.N, dtype=torch.float64)
        return form_product(self.form, self.a, self.b, k0, k1)

    def logical_mask(self):
        m = torch.zeros(self.c_buf.numel(), dtype=torch.bool)
        for s in range(self.slabs):
            o = self.c_off + s * self.slab_stride
            m[o:o + self.M * self.ldc].view(self.M, self.ldc)[:, :self.N] = True
        return m

    def logical(self, c_flat):
        """[slabs, M, N] copy of the logical blocks of a C buffer."""
        out = []
        for s in range(self.slabs):
            o = self.c_off + s * self.slab_stride
            out.append(c_flat[o:o + self.M * self.ldc].view(self.M, self.ldc)[:, :self.N].clone())
        return torch.stack(out)

    def with_c0(self, c0):
        """A C buffer whose logical block holds `c0` (accumulate), sentinel elsewhere."""
        assert self.slabs == 1
        buf = self.c_buf.clone()
        buf[self.c_off:self.c_off + self.M * self.ldc].view(self.M, self.ldc)[:, :self.N] = c0.to(buf.dtype)
        return buf

    def assert_padding_untouched(self, c_flat):
        """Every padding, gap and guard element of C still holds the sentinel, bit for bit."""
        assert c_flat.dtype == self.c_buf.dtype and c_flat.numel() == self.c_buf.numel()
        out = ~self.logical_mask()
        bad = (bits(c_flat)[out] != bits(self.c_buf)[out]).nonzero().flatten()
        assert bad.numel() == 0, (f'{bad.numel()} padding / guard elements of C overwritten, first at flat index '
                                  f'{int(out.nonzero().flatten()[bad[0]])} (C starts at {self.c_off}, ldc {self.ldc})')


def operands(form, M, N, K, kind, seed):
    """Logical operands as stored.  'int': A from randint(-4, 5), B = (arange % 13) - 6 -- with K <= 200 every partial sum
    stays below 4 * 6 * 200 < 2^24, so the product is exact in fp32 in ANY summation order.  'int1': randint(-1, 2) on both
    sides (bf16 outputs: exact in bf16 too).  'intw': B = 16 ((arange % 13) - 6) + 1, odd integers up to 97 (exact in bf16):
    sums below 4 * 97 * 200 < 2^24, still exact in fp32, but in the thousands with live low bits -- a bf16 output has to
    ROUND nearly every element, once.  'rand': randn rounded to bf16."""
    g = torch.Generator().manual_seed(seed)
    sa, sb = _stored_shapes(form, M, N, K)
    if kind == 'int':
        a = torch.randint(-4, 5, sa, generator=g).float()
        b = (torch.arange(sb[0] * sb[1], dtype=torch.float32).reshape(sb) % 13) - 6
    elif kind == 'intw':
        a = torch.randint(-4, 5, sa, generator=g).float()
        b = ((torch.arange(sb[0] * sb[1], dtype=torch.float32).reshape(sb) % 13) - 6) * 16 + 1
    elif kind == 'int1':
        a = torch.randint(-1, 2, sa, generator=g).float()
        b = torch.randint(-1, 2, sb, generator=g).float()
    elif kind == 'rand':
        a, b = torch.randn(sa, generator=g), torch.randn(sb, generator=g)
    else:
        raise ValueError(kind)
    return a.to(torch.bfloat16), b.to(torch.bfloat16)


def c_buffer(M, N, pc, slabs=1, bf16=False):
    """Sentinel-filled C storage: one guard row, `slabs` slabs of M rows with leading dimension N + pc (SLAB_GAP sentinel
    elements more between two slabs, slab_stride a multiple of 4), one guard row."""
    ldc = N + pc
    stride = -(-(M * ldc) // 4) * 4 + SLAB_GAP
    n = ldc + slabs * stride + ldc
    if bf16:
        buf = torch.full((n,), BF16_SENTINEL, dtype=torch.int16).view(torch.bfloat16)
    else:
        buf = torch.full((n,), float('nan'))
    return buf, ldc, ldc, stride


def make_case(form, M, N, K, pads=(0, 0, 0), seed=0, kind='int', slabs=1, c_bf16=False):
    """The four things a device test needs: operands in padded storage, the sentinel-filled C buffer, the float64
    reference and (Case.assert_padding_untouched) the check that nothing but the logical block of C was written."""
    assert form in FORMS
    pa, pb, pc = pads
    a, b = operands(form, M, N, K, kind, seed)
    a_buf, lda = pad_operand(a, pa)
    b_buf, ldb = pad_operand(b, pb)
    c_buf, ldc, c_off, stride = c_buffer(M, N, pc, slabs, c_bf16)
    case = Case(form, M, N, K, kind, a, b, a_buf, b_buf, lda, ldb, ldc, c_buf, c_off, slabs, stride, None)
    case.ref = case.product()
    return case


def rne_bf16(ref64):
    """Expected bf16 output of an integer case: ONE round-to-nearest-even of the exact fp32 value."""
    f = ref64.float()
    assert torch.equal(f.double(), ref64), 'the reference must be exactly representable in fp32'
    return f.to(torch.bfloat16)


def tile_partials(ref_fp64, BM, BN):
    """Per-tile sums of squares of an [M, N] matrix in the documented slot order (include/jamie_hip.h): tile (i, j) --
    rows i * BM .., columns j * BN .. -- at slot i + tiles_m * j."""
    M, N = ref_fp64.shape
    tm, tn = math.ceil(M / BM), math.ceil(N / BN)
    out = torch.zeros(tm * tn, dtype=torch.float64)
    for j in range(tn):
        for i in range(tm):
            out[i + tm * j] = (ref_fp64[i * BM:(i + 1) * BM, j * BN:(j + 1) * BN].double() ** 2).sum()
    return out


def random_tolerance(K):
    """test_gemm_bf16's: exact bf16 products, fp32 accumulation."""
    return 1e-5, 1.2e-5 * float(np.sqrt(K))


def error_ratio(out, ref, rtol, atol):
    """(largest |out - ref|, largest |out - ref| / (atol + rtol |ref|)); a NaN anywhere gives (nan, inf)."""
    out, ref = out.double(), ref.double()
    if not bool(torch.isfinite(out).all()):
        return float('nan'), float('inf')
    err = (out - ref).abs()
    return float(err.max()), float((err / (atol + rtol * ref.abs())).max())


# ---- the grouped launches of test 7 ------------------------------------------------------------------------------------
# tile counts 1, 3, 5, 7, 2, 9, 11 and 4, in an order in which no prefix sums to a multiple of 8 (1, 4, 9, 11, 18, 27, 38;
# total 42): every problem after the first starts on a rotated XCD, every `rp` of the decode differs from 0
GROUP_COUNTS = [1, 3, 5, 2, 7, 9, 11, 4]


def mixed_group(BM=128, BN=128):
    """(form, M, N, K, splitk, (tiles_m, tiles_n)) of the backward-like group on configuration 29: dX (b_tr, splitk 2: the tile
    count doubles), dW (a_tr + b_tr with partial, store_nt, c_bf16) and one plain NT."""
    return [('a_tr_b_tr', 72, 40, 72, 1, (1, 1)),
            ('nt', 2 * BM + 8, BN - 6, 72, 1, (3, 1)),
            ('a_tr_b_tr', 4 * BM + 8, 72, 64, 1, (5, 1)),
            ('b_tr', BM - 8, 72, 136, 2, (1, 1)),
            ('a_tr_b_tr', BM, 6 * BN + 8, 200, 1, (1, 7)),
            ('a_tr_b_tr', 2 * BM + 8, 2 * BN + 8, 24, 1, (3, 3)),
            ('a_tr_b_tr', 10 * BM + 8, 120, 72, 1, (11, 1)),
            ('b_tr', BM + 8, BN, 72, 2, (2, 1))]


def nt_group(BM, BN):
    """Eight NT problems with the same tile counts (configurations 31 and 32)."""
    fact = [(1, 1), (3, 1), (1, 5), (2, 1), (7, 1), (3, 3), (11, 1), (2, 2)]
    tail_m = [8, 1, 40, 9, 8, 33, 8, 127]
    tail_n = [8, 2, 3, 64, 12, 8, 5, 66]
    ks = [72, 64, 24, 200, 72, 136, 8, 72]
    return [('nt', (tm - 1) * BM + dm, (tn - 1) * BN + dn, k, 1, (tm, tn))
            for (tm, tn), dm, dn, k in zip(fact, tail_m, tail_n, ks)]


def group_tiles(group, BM, BN):
    return [math.ceil(M / BM) * math.ceil(N / BN) * sk for (_, M, N, _, sk, _) in group]

// Sparse PCA products, gfx950: the three products randomized PCA asks of the centred cells Xc = X - 1 mean^T (jamie_amd/pca.py),
// taken from the CSR / CSC arrays of X with the centring as a rank-one correction in the epilogue:
//     Xc Q = X Q - 1 (mean^T Q),   Xc^T Y = X^T Y - mean (1^T Y),   Xc V^T = X V^T - 1 (mean^T V^T).
// jamie_csr_spmm is the sparse x dense product, jamie_weighted_colsum gives the row vector t of the correction.
// A wave owns a row (or one segment of a long row); its lanes span the output columns, each with ceil(n / 64) fp32 accumulators in
// registers.  64 (index, value) pairs are read at a time, one per lane, and handed round with v_readlane, so the row B[idx, :] is
// addressed from scalar registers and read as one contiguous line per 64 columns.
// Deterministic and row-local: the stored entries of a row are added in their stored order; a row of more than SPMM_SEG entries is
// cut into segments of SPMM_SEG counted from its own start, every segment gives one fp32 partial [n] in the workspace and the
// partials are added in ascending order.  No floating-point atomics.
#include "common.h"

#define SPMM_SEG 2048           // stored entries per segment of a long row (jamie_amd/sparse_pca.py: SEGMENT)
#define SPMM_MAX_NA 16          // accumulators per lane of one panel: panels of 64 * 16 = 1024 output columns
#define WCS_ROWS 512            // rows per fp64 partial of jamie_weighted_colsum (sparse_pca.py: COLSUM_ROWS)

// ---- workspace --------------------------------------------------------------------------------------------------------------
// The partial of a segment lives in a slot that is found from the POSITIONS of the row's entries alone, so that neither side needs
// a scan over the row pointers: positions are cut into windows of SPMM_SEG, window w has the slots 2w and 2w + 1.  A long row
// [b, e) touches the windows w0 = b / SEG .. w1 = (e - 1) / SEG, c = w1 - w0 + 1 >= 2 of them, and has ceil((e - b) / SEG) <= c
// segments.  Segment i < c - 1 takes slot 2 (w0 + 1 + i): a window the row reaches from the left, which no other row does.
// Segment c - 1, if there is one, takes slot 2 w0 + 1: the window the row starts in, and only one long row starts in a window.
__host__ __device__ inline long long spmm_windows(long long nnz) { return nnz > SPMM_SEG ? (nnz + SPMM_SEG - 1) / SPMM_SEG : 0; }

extern "C" long long jamie_spmm_workspace(const long long* ptr, long long n_rows, int n) {
    if (!ptr || n_rows < 1 || n < 1) return 0;
    for (long long r = 0; r < n_rows; ++r)
        if (ptr[r + 1] < ptr[r]) return 0;
    if (ptr[0] < 0) return 0;
    return 8LL * n * spmm_windows(ptr[n_rows]);
}

__device__ __forceinline__ long long spmm_clamp(long long v, long long nnz) { return max(0LL, min(v, nnz)); }

// acc[a] += sum over the stored entries p in [pb, pe), in ascending p, of (float)vals[p] * B[idx[p], col[a]].  Wave-uniform
// arguments but for `lane` and `col` (columns clamped to n - 1 by the caller: the lanes beyond n compute a value nobody stores).
// An index outside [0, n_inner) is skipped.  Both loops below add the same terms in the same order with the same fmaf.
template <typename T, int NA>
__device__ __forceinline__ void spmm_range(const int32_t* __restrict__ idx, const T* __restrict__ vals, long long pb, long long pe,
                                           long long n_inner, const float* __restrict__ B, long long ld_b, int lane,
                                           const int (&col)[NA], float (&acc)[NA]) {
    for (long long p0 = pb; p0 < pe; p0 += 64) {
        const long long p = p0 + lane;
        int c = 0;
        float v = 0.f;
        bool ok = false;
        if (p < pe) {
            c = idx[p];
            v = (float)vals[p];
            ok = c >= 0 && (long long)c < n_inner;
        }
        const unsigned long long mask = __builtin_amdgcn_ballot_w64(ok);
        const int vi = __builtin_bit_cast(int, v);
        if (mask == ~0ULL) {
#pragma unroll 8
            for (int q = 0; q < 64; ++q) {
                const int cq = __builtin_amdgcn_readlane(c, q);
                const float vq = __builtin_bit_cast(float, __builtin_amdgcn_readlane(vi, q));
                const float* __restrict__ row = B + (long long)cq * ld_b;
#pragma unroll
                for (int a = 0; a < NA; ++a) acc[a] = __builtin_fmaf(vq, row[col[a]], acc[a]);
            }
        } else {
            unsigned long long m = mask;                   // a ragged or partly invalid group: the valid lanes in ascending order
            while (m) {
                const int q = __builtin_ctzll(m);
                m &= m - 1;
                const int cq = __builtin_amdgcn_readlane(c, q);
                const float vq = __builtin_bit_cast(float, __builtin_amdgcn_readlane(vi, q));
                const float* __restrict__ row = B + (long long)cq * ld_b;
#pragma unroll
                for (int a = 0; a < NA; ++a) acc[a] = __builtin_fmaf(vq, row[col[a]], acc[a]);
            }
        }
    }
}

// ---- one wave per slot: the partial of the long-row segment that owns the slot, if any ----
template <typename T, int NA>
__global__ __launch_bounds__(256) void spmm_segment_kernel(const long long* __restrict__ ptr, const int32_t* __restrict__ idx,
                                                           const T* __restrict__ vals, long long nnz, long long n_rows,
                                                           long long n_inner, const float* __restrict__ B, long long ld_b, int n,
                                                           float* __restrict__ partials, long long n_slots) {
    const int lane = threadIdx.x & 63;
    const long long u = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (u >= n_slots) return;
    const long long w = u >> 1, pos = ((u + 1) >> 1) * SPMM_SEG;     // the owner holds position pos: w SEG (even), (w + 1) SEG (odd)
    if (pos >= nnz) return;
    long long lo = 0, hi = n_rows;                                   // the last row that starts at or before pos
    while (hi - lo > 1) {
        const long long mid = (lo + hi) >> 1;
        if (spmm_clamp(ptr[mid], nnz) <= pos) lo = mid; else hi = mid;
    }
    const long long b = spmm_clamp(ptr[lo], nnz), e = max(b, spmm_clamp(ptr[lo + 1], nnz));
    if (e - b <= SPMM_SEG || e <= pos) return;
    const long long w0 = b / SPMM_SEG, w1 = (e - 1) / SPMM_SEG, nseg = (e - b + SPMM_SEG - 1) / SPMM_SEG;
    long long i;
    if (u & 1) {
        if (w0 != w) return;
        i = w1 - w0;
    } else {
        if (b >= pos) return;
        i = w - w0 - 1;
    }
    if (i < 0 || i >= nseg) return;
    const long long pb = b + i * SPMM_SEG, pe = min(e, pb + SPMM_SEG);
    float* __restrict__ o = partials + u * n;
    for (int j0 = 0; j0 < n; j0 += 64 * NA) {
        int col[NA];
        float acc[NA];
#pragma unroll
        for (int a = 0; a < NA; ++a) { col[a] = min(j0 + lane + 64 * a, n - 1); acc[a] = 0.f; }
        spmm_range<T, NA>(idx, vals, pb, pe, n_inner, B, ld_b, lane, col, acc);
#pragma unroll
        for (int a = 0; a < NA; ++a) {
            const int j = j0 + lane + 64 * a;
            if (j < n) o[j] = acc[a];
        }
    }
}

// ---- one wave per row: the product of a short row, or the sum of a long row's partials; then the rank-one correction ----
template <typename T, int NA>
__global__ __launch_bounds__(256) void spmm_row_kernel(const long long* __restrict__ ptr, const int32_t* __restrict__ idx,
                                                       const T* __restrict__ vals, long long nnz, long long n_rows, long long n_inner,
                                                       const float* __restrict__ B, long long ld_b, int n,
                                                       const double* __restrict__ s, const float* __restrict__ t,
                                                       float* __restrict__ out, long long ld_out,
                                                       const float* __restrict__ partials, long long n_slots) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (r >= n_rows) return;
    const long long b = spmm_clamp(ptr[r], nnz), e = max(b, spmm_clamp(ptr[r + 1], nnz));
    const float sr = s ? (float)s[r] : 1.f;
    float* __restrict__ o = out + r * ld_out;
    for (int j0 = 0; j0 < n; j0 += 64 * NA) {
        int col[NA];
        float acc[NA];
#pragma unroll
        for (int a = 0; a < NA; ++a) { col[a] = min(j0 + lane + 64 * a, n - 1); acc[a] = 0.f; }
        if (e - b <= SPMM_SEG) {
            spmm_range<T, NA>(idx, vals, b, e, n_inner, B, ld_b, lane, col, acc);
        } else {
            const long long w0 = b / SPMM_SEG, w1 = (e - 1) / SPMM_SEG, nseg = (e - b + SPMM_SEG - 1) / SPMM_SEG;
            for (long long i = 0; i < nseg; ++i) {                          // ascending segments
                const long long slot = i < w1 - w0 ? 2 * (w0 + 1 + i) : 2 * w0 + 1;
                if (slot >= n_slots) break;                                 // (cannot happen: the entry point checks the workspace)
                const float* __restrict__ ps = partials + slot * n;
#pragma unroll
                for (int a = 0; a < NA; ++a) acc[a] += ps[col[a]];
            }
        }
#pragma unroll
        for (int a = 0; a < NA; ++a) {
            const int j = j0 + lane + 64 * a;
            if (j < n) o[j] = t ? __builtin_fmaf(-sr, t[j], acc[a]) : acc[a];          // one rounding for product and subtraction
        }
    }
}

template <typename T, int NA>
static void spmm_launch(const long long* ptr, const int32_t* idx, const void* vals, long long nnz, long long n_rows, long long n_inner,
                        const float* B, long long ld_b, int n, const double* s, const float* t, float* out, long long ld_out,
                        float* partials, long long n_slots, hipStream_t st) {
    if (n_slots > 0)
        hipLaunchKernelGGL((spmm_segment_kernel<T, NA>), dim3((unsigned)((n_slots + 3) / 4)), dim3(256), 0, st, ptr, idx, (const T*)vals,
                           nnz, n_rows, n_inner, B, ld_b, n, partials, n_slots);
    hipLaunchKernelGGL((spmm_row_kernel<T, NA>), dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, st, ptr, idx, (const T*)vals, nnz,
                       n_rows, n_inner, B, ld_b, n, s, t, out, ld_out, partials, n_slots);
}

#define SPMM_CASE(NA)                                                                                                              \
    if (na <= NA) {                                                                                                                \
        if (is_f64) spmm_launch<double, NA>(ptr, idx, vals, nnz, n_rows, n_inner, B, ld_b, n, s, t, out, ld_out, part, n_slots, st); \
        else spmm_launch<float, NA>(ptr, idx, vals, nnz, n_rows, n_inner, B, ld_b, n, s, t, out, ld_out, part, n_slots, st);       \
        return jamie_launch_status("jamie_csr_spmm");                                                                              \
    }

extern "C" int jamie_csr_spmm(const long long* ptr, const int32_t* idx, const void* vals, int is_f64, long long nnz, long long n_rows,
                              long long n_inner, const float* B, long long ld_b, int n, const double* s, const float* t, float* out,
                              long long ld_out, void* ws, long long ws_bytes, void* stream) {
    JAMIE_ARG(ptr && B && out && n_rows >= 0 && n_inner >= 1 && n >= 1, "null pointer / n_inner < 1 / n < 1");
    JAMIE_ARG(ld_b >= n && ld_out >= n, "ld_b < n or ld_out < n");
    JAMIE_ARG(nnz >= 0 && (nnz == 0 || (idx && vals)), "nnz > 0 needs indices and values");
    const long long n_slots = 2 * spmm_windows(nnz);
    JAMIE_ARG(n_slots == 0 || (ws && ws_bytes >= 4LL * n * n_slots && (uintptr_t)ws % 4 == 0),
              "workspace smaller than jamie_spmm_workspace(ptr, n_rows, n) or misaligned");
    JAMIE_ARG((n_rows + 3) / 4 <= 0x7fffffffLL && (n_slots + 3) / 4 <= 0x7fffffffLL, "n_rows, nnz / 1024 <= 4 * (2^31 - 1)");
    if (n_rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    float* part = (float*)ws;
    const int na = (min(n, 64 * SPMM_MAX_NA) + 63) / 64;               // accumulators per lane; wider outputs go panel by panel
    SPMM_CASE(1) SPMM_CASE(2) SPMM_CASE(3) SPMM_CASE(4) SPMM_CASE(6) SPMM_CASE(9) SPMM_CASE(12) SPMM_CASE(16)
    return jamie_fail(-1, "%s: no kernel for n = %lld", "jamie_csr_spmm", n);
}

// ---- t[j] = sum_r w[r] B[r, j] in fp64: one partial per WCS_ROWS rows (four interleaved row lanes, combined as (0 + 1) + (2 + 3)),
//      the partials added in ascending order, one rounding to fp32 ----
__global__ __launch_bounds__(256) void wcs_partial_kernel(const float* __restrict__ B, long long rows, int n, long long ld_b,
                                                          const double* __restrict__ w, double* __restrict__ part) {
    __shared__ double sh[4][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int j = blockIdx.y * 64 + tx;
    const long long r0 = (long long)blockIdx.x * WCS_ROWS, r1 = min(rows, r0 + WCS_ROWS);
    double acc = 0.0;
    if (j < n) {
        if (w) for (long long r = r0 + ty; r < r1; r += 4) acc += w[r] * (double)B[r * ld_b + j];
        else for (long long r = r0 + ty; r < r1; r += 4) acc += (double)B[r * ld_b + j];
    }
    sh[ty][tx] = acc;
    __syncthreads();
    if (ty == 0 && j < n) part[(long long)blockIdx.x * n + j] = (sh[0][tx] + sh[1][tx]) + (sh[2][tx] + sh[3][tx]);
}

__global__ __launch_bounds__(256) void wcs_finish_kernel(const double* __restrict__ part, long long chunks, int n, float* __restrict__ t) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    double s = 0.0;
    for (long long c = 0; c < chunks; ++c) s += part[c * n + j];
    t[j] = (float)s;
}

extern "C" int jamie_weighted_colsum(const float* B, long long rows, int n, long long ld_b, const double* w, float* t, void* ws,
                                     long long ws_bytes, void* stream) {
    JAMIE_ARG(B && t && rows >= 1 && n >= 1 && ld_b >= n, "null pointer / empty / ld_b < n");
    const long long chunks = (rows + WCS_ROWS - 1) / WCS_ROWS;
    JAMIE_ARG(ws && ws_bytes >= 8LL * n * chunks && (uintptr_t)ws % 8 == 0, "workspace smaller than 8 n ceil(rows / 512) or misaligned");
    JAMIE_ARG(chunks <= 0x7fffffffLL && (n + 63) / 64 <= 65535, "rows <= 512 * (2^31 - 1), n <= 64 * 65535");
    hipStream_t st = (hipStream_t)stream;
    double* part = (double*)ws;
    hipLaunchKernelGGL(wcs_partial_kernel, dim3((unsigned)chunks, (unsigned)((n + 63) / 64)), dim3(256), 0, st, B, rows, n, ld_b, w, part);
    hipLaunchKernelGGL(wcs_finish_kernel, dim3((n + 255) / 256), dim3(256), 0, st, part, chunks, n, t);
    return jamie_launch_status("jamie_weighted_colsum");
}

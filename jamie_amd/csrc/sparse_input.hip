// Sparse (CSR) cell matrices, gfx950: the per-feature statistics of `preclass(axis=0)` (reference utilities.py:654-678, built at
// jamie.py:462-465) from the stored entries alone, and the standardised dense fp32 rows (jamie.py:508, 806-837) the training loop
// and the eval GEMMs consume, written straight from the CSR arrays.  No dense copy of the input exists on either side.
// Deterministic: fp64 partial sums per fixed-length segment of a column, added in ascending order; no floating-point atomics.
#include "common.h"

#define SP_SEG 4096            // stored entries per statistics segment (jamie_amd/sparse_input.py: SEGMENT)
#define SP_WIN 4096            // columns of one LDS window (sparse_input.py: WINDOW)
#define SP_ROWS 2              // rows held in LDS at a time: 2 x 4096 floats = 32 KB
#define SP_ROWS_PER_WG 16      // rows one workgroup walks through, SP_ROWS at a time

// host arithmetic only.  which = 0: the fp64 segment partials of jamie_csc_col_stats for this (host) colptr; 1: the structural-zero
// row of jamie_csr_standardise
extern "C" long long jamie_sparse_workspace(const long long* colptr, int d, int which) {
    if (d < 1) return 0;
    if (which == 1) return 4LL * d;
    if (which != 0 || !colptr) return 0;
    long long segs = 0;
    for (int c = 0; c < d; ++c) {
        const long long n = colptr[c + 1] - colptr[c];
        if (n < 0) return 0;
        segs += (n + SP_SEG - 1) / SP_SEG;
    }
    return 8 * segs;
}

// ---- one workgroup per segment: partials[t] = sum v (mean == NULL) or sum (v - mean[c])^2 over the segment's stored entries ----
template <typename T>
__global__ __launch_bounds__(256) void csc_moment_kernel(const T* __restrict__ vals, long long nnz, const long long* __restrict__ colptr,
                                                         const long long* __restrict__ seg_off, int d,
                                                         const double* __restrict__ mean, double* __restrict__ partials) {
    __shared__ double sh[256];
    const long long t = blockIdx.x;
    int lo = 0, hi = d;                                    // seg_off[lo] <= t < seg_off[hi]: the column that owns segment t
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (seg_off[mid] <= t) lo = mid; else hi = mid;
    }
    const int c = lo;
    long long b = colptr[c] + (t - seg_off[c]) * SP_SEG;
    long long e = min(colptr[c + 1], b + SP_SEG);
    b = max(b, 0LL);
    e = min(e, nnz);
    double acc = 0.0;
    if (mean) {
        const double mu = mean[c];
        for (long long i = b + threadIdx.x; i < e; i += 256) { const double v = (double)vals[i] - mu; acc += v * v; }
    } else {
        for (long long i = b + threadIdx.x; i < e; i += 256) acc += (double)vals[i];
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) partials[t] = sh[0];
}

// a column's partials in ascending segment order; mean = sum / N, sd = sqrt((sum dev^2 + (N - n_c) mean^2) / N): the structural
// zeros deviate by -mean each.  Divisions by N (not a product with 1 / N): N equal stored values give their value and sd = 0 exactly
__global__ __launch_bounds__(256) void csc_finish_kernel(const double* __restrict__ partials, const long long* __restrict__ colptr,
                                                         const long long* __restrict__ seg_off, long long N, int d, int pass,
                                                         double* mean, double* sd) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= d) return;
    double s = 0.0;
    for (long long t = seg_off[c]; t < seg_off[c + 1]; ++t) s += partials[t];
    if (!pass) {
        mean[c] = s / (double)N;
    } else {
        const double mu = mean[c];
        const double absent = (double)(N - (colptr[c + 1] - colptr[c]));
        sd[c] = sqrt((s + absent * (mu * mu)) / (double)N);
    }
}

extern "C" int jamie_csc_col_stats(const void* vals, int is_f64, long long nnz, const long long* colptr, const long long* seg_off,
                                   long long n_seg, long long N, int d, double* mean, double* sd, void* ws, long long ws_bytes,
                                   void* stream) {
    JAMIE_ARG(colptr && seg_off && mean && sd && N > 0 && d > 0, "null pointer / empty");
    JAMIE_ARG(nnz >= 0 && n_seg >= 0 && n_seg <= 0x7fffffffLL && n_seg <= nnz, "0 <= n_seg <= nnz, n_seg < 2^31");
    JAMIE_ARG(n_seg == 0 || (vals && ws && ws_bytes >= 8 * n_seg), "workspace smaller than jamie_sparse_workspace(colptr, d, 0)");
    hipStream_t st = (hipStream_t)stream;
    double* partials = (double*)ws;
    const dim3 fin((d + 255) / 256);
    for (int pass = 0; pass < 2; ++pass) {
        const double* mu = pass ? mean : nullptr;
        if (n_seg > 0) {
            if (is_f64) hipLaunchKernelGGL(csc_moment_kernel<double>, dim3((unsigned)n_seg), dim3(256), 0, st, (const double*)vals, nnz, colptr, seg_off, d, mu, partials);
            else hipLaunchKernelGGL(csc_moment_kernel<float>, dim3((unsigned)n_seg), dim3(256), 0, st, (const float*)vals, nnz, colptr, seg_off, d, mu, partials);
        }
        hipLaunchKernelGGL(csc_finish_kernel, fin, dim3(256), 0, st, partials, colptr, seg_off, N, d, pass, mean, sd);
    }
    return jamie_launch_status("jamie_csc_col_stats");
}

// ---- z[c] = what a cell without a stored entry in feature c standardises to: standardise_kernel's expression (misc.hip) at x = 0 ----
__global__ __launch_bounds__(256) void zero_row_kernel(const double* __restrict__ mean, const double* __restrict__ sd, int d,
                                                       float* __restrict__ z) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= d) return;
    const double v = ((double)0.f - mean[c]) / sd[c];
    z[c] = (v != v) ? 0.f : (float)v;
}

// A workgroup walks SP_ROWS_PER_WG rows of one window of SP_WIN columns, SP_ROWS rows at a time: the window rows are filled from z
// in LDS, the stored entries that fall into the window (found by a lower_bound on the row's sorted column indices) overwrite their
// slots with the standardised stored value, and the rows leave with one contiguous store each: every element of `out` is written
// exactly once.  A stored index outside [0, d) is never written (the slot test is on the window, which ends at d), row extents are
// clamped to [0, nnz].
template <typename T>
__global__ __launch_bounds__(256) void csr_standardise_kernel(const long long* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                              const T* __restrict__ vals, long long nnz, long long n_rows, int d,
                                                              const double* __restrict__ mean, const double* __restrict__ sd,
                                                              const float* __restrict__ z, float* __restrict__ out, long long ld_out) {
    __shared__ __attribute__((aligned(16))) float win[SP_ROWS][SP_WIN];
    const int tid = threadIdx.x;
    const int c0 = blockIdx.y * SP_WIN;
    const int wlen = min(SP_WIN, d - c0), c1 = c0 + wlen;
    const int nq = wlen >> 2;
    const long long rb = (long long)blockIdx.x * SP_ROWS_PER_WG;
    for (int it = 0; it < SP_ROWS_PER_WG; it += SP_ROWS) {
        const long long r0 = rb + it;
        if (r0 >= n_rows) break;                                               // (uniform)
        // fill: z + c0 is 16-byte aligned (c0 is a multiple of SP_WIN, z checked by the entry point)
        for (int q = tid; q < nq; q += 256) {
            const float4 v = reinterpret_cast<const float4*>(z + c0)[q];
#pragma unroll
            for (int r = 0; r < SP_ROWS; ++r) reinterpret_cast<float4*>(win[r])[q] = v;
        }
        for (int i = (nq << 2) + tid; i < wlen; i += 256) {
            const float v = z[c0 + i];
#pragma unroll
            for (int r = 0; r < SP_ROWS; ++r) win[r][i] = v;
        }
        __syncthreads();
        // stored entries: 256 / SP_ROWS threads per row
        {
            const int per = 256 / SP_ROWS, r = tid / per, t = tid % per;
            const long long row = r0 + r;
            if (row < n_rows) {
                long long beg = indptr[row], end = indptr[row + 1];
                beg = max(0LL, min(beg, nnz));
                end = max(beg, min(end, nnz));
                long long lo = beg;
                if (c0 > 0) {
                    long long hi = end;
                    while (lo < hi) {
                        const long long mid = (lo + hi) >> 1;
                        if (indices[mid] < c0) lo = mid + 1; else hi = mid;
                    }
                }
                for (long long j = lo + t; j < end; j += per) {
                    const int c = indices[j];
                    if (c >= c1) break;                                        // sorted: the rest lies right of the window
                    if (c >= c0) {
                        const double v = ((double)vals[j] - mean[c]) / sd[c];  // utilities.py:663-668, as standardise_kernel
                        win[r][c - c0] = (v != v) ? 0.f : (float)v;
                    }
                }
            }
        }
        __syncthreads();
        // store: scalar head up to the first 16-byte boundary of the output row, float4 body, scalar tail
#pragma unroll
        for (int r = 0; r < SP_ROWS; ++r) {
            const long long row = r0 + r;
            if (row >= n_rows) break;
            float* o = out + row * ld_out + c0;
            int head = (int)((4 - (((uintptr_t)o >> 2) & 3)) & 3);
            if (head > wlen) head = wlen;
            const int nqs = (wlen - head) >> 2;
            if (tid < head) o[tid] = win[r][tid];
            if (head == 0) {
                for (int q = tid; q < nqs; q += 256) reinterpret_cast<float4*>(o)[q] = reinterpret_cast<const float4*>(win[r])[q];
            } else {
                for (int q = tid; q < nqs; q += 256) {
                    const float* s = &win[r][head + 4 * q];
                    reinterpret_cast<float4*>(o + head)[q] = make_float4(s[0], s[1], s[2], s[3]);
                }
            }
            for (int i = head + (nqs << 2) + tid; i < wlen; i += 256) o[i] = win[r][i];
        }
        __syncthreads();                                                       // the next fill overwrites the window
    }
}

extern "C" int jamie_csr_standardise(const long long* indptr, const int32_t* indices, const void* vals, int is_f64, long long nnz,
                                     long long n_rows, int d, const double* mean, const double* sd, float* out, long long ld_out,
                                     void* ws, long long ws_bytes, void* stream) {
    JAMIE_ARG(indptr && mean && sd && out && ws && n_rows > 0 && d > 0 && ld_out >= d, "null pointer / empty / ld_out < d");
    JAMIE_ARG(nnz >= 0 && (nnz == 0 || (indices && vals)), "nnz > 0 needs indices and values");
    JAMIE_ARG(ws_bytes >= 4LL * d && (uintptr_t)ws % 16 == 0 && (uintptr_t)out % 4 == 0, "workspace smaller than jamie_sparse_workspace(0, d, 1) or misaligned");
    const long long gx = (n_rows + SP_ROWS_PER_WG - 1) / SP_ROWS_PER_WG;
    const int gy = (d + SP_WIN - 1) / SP_WIN;
    JAMIE_ARG(gx <= 0x7fffffffLL && gy <= 65535, "n_rows <= 16 * (2^31 - 1), d <= 65535 * 4096");
    hipStream_t st = (hipStream_t)stream;
    float* z = (float*)ws;
    hipLaunchKernelGGL(zero_row_kernel, dim3((d + 255) / 256), dim3(256), 0, st, mean, sd, d, z);
    const dim3 grid((unsigned)gx, (unsigned)gy);
    if (is_f64) hipLaunchKernelGGL(csr_standardise_kernel<double>, grid, dim3(256), 0, st, indptr, indices, (const double*)vals, nnz, n_rows, d, mean, sd, z, out, ld_out);
    else hipLaunchKernelGGL(csr_standardise_kernel<float>, grid, dim3(256), 0, st, indptr, indices, (const float*)vals, nnz, n_rows, d, mean, sd, z, out, ld_out);
    return jamie_launch_status("jamie_csr_standardise");
}

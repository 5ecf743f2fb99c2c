// Spectral embedding on the device (include/jamie_hip.h "Spectral embedding on the device"; jamie_amd/spectral.py): the products a
// Chebyshev-filtered subspace iteration needs on the CSR fuzzy graph of umap.hip and on [N, B] fp64 blocks, B = 16 or 32 columns,
// row-major (a row of the block is one or two 128-byte lines).  O(nnz + N B) memory.  DESIGN.md §21.
//
//   spectral_rowsum_kernel   16 lanes per row of the graph: sum_j A_ij w_j in fp64
//   spectral_cheb_kernel     B lanes per row, lane l owns column l: out = alpha s_i sum_j A_ij s_j in[j, l] + gamma in - beta prev
//   spectral_gram_kernel     one workgroup per segment of 512 rows: its part of Y^T Z; spectral_gram_sum_kernel adds the parts
//   spectral_rotate_kernel   B lanes per row: out = Y1 M1 (+ Y2 M2), the B x B matrices in LDS
//
// Deterministic: no atomics; every sum has one owner and a fixed order.
#include "lane_tree.h"

namespace {

constexpr int SP_GROUP = 16;           // lanes that own a row in the row sum
constexpr int SP_GRAM_ROWS = 512;      // rows of a Gram segment: fixed, whatever the device
constexpr int SP_GRAM_TILE = 64;       // rows staged in LDS at a time

// ---- degree: out_i = sum_j A_ij w_j ----
// lane l of the row's 16 adds entries l, l + 16, ... in ascending order (product, then sum: no contraction); the 16 partial sums by
// the xor tree 8, 4, 2, 1
__global__ __launch_bounds__(256) void spectral_rowsum_kernel(const long long* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                              const float* __restrict__ val, const double* __restrict__ w,
                                                              long long N, long long nnz, double* __restrict__ out) {
#pragma clang fp contract(off)
    const int l = threadIdx.x & (SP_GROUP - 1);
    const long long row = (long long)blockIdx.x * (256 / SP_GROUP) + (threadIdx.x / SP_GROUP);
    const bool live = row < N;
    long long e0 = 0, e1 = 0;
    if (live) {
        e0 = rowptr[row];
        e1 = rowptr[row + 1];
        e0 = e0 < 0 ? 0 : e0;
        e1 = e1 > nnz ? nnz : e1;
    }
    double acc = 0.0;
    for (long long e = e0 + l; e < e1; e += SP_GROUP) {
        const long long j = col[e];
        if (j < 0 || j >= N) continue;
        const double a = (double)val[e];
        acc = acc + (w ? a * w[j] : a);
    }
    for (int s = SP_GROUP / 2; s > 0; s >>= 1) acc = acc + __shfl_xor(acc, s);      // (every lane of the wave is here)
    if (live && l == 0) out[row] = acc;
}

// ---- the hot path: one step of the three-term recurrence on the scaled graph ----
// B lanes own row i; lane l owns column l.  For the entries of the row in ascending order, j = col[e]:
//   acc = acc + ((double)val[e] * scale[j]) * in[j, l]                       (two products, one sum; no contraction)
// then out[i, l] = ((alpha * scale[i]) * acc + gamma * in[i, l]) - beta * prev[i, l]   (the last term only with prev).
// The row is walked B entries at a time: lane l of the group loads entry base + l -- its column and val * scale[column] -- once,
// and the group reads the B pairs from one another by __shfl (width B) in entry order, each lane gathering its own double of row j
// of `in` (B consecutive doubles per group: one or two 128-byte lines).  SP_DEPTH gathers are issued before their sums are taken.
// The lanes of a group take every branch together (their trip counts are the row's), so every __shfl reads a lane that is
// active.  No LDS allocation, no scratch, no atomics.
constexpr int SP_DEPTH = 8;

template <int B>
__global__ __launch_bounds__(256) void spectral_cheb_kernel(const long long* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                            const float* __restrict__ val, long long nnz,
                                                            const double* __restrict__ scale, const double* __restrict__ in,
                                                            const double* prev, double* out, long long N, double alpha, double gamma,
                                                            double beta) {
#pragma clang fp contract(off)
    static_assert(B % SP_DEPTH == 0, "a pass over B entries is a whole number of batches");
    const int l = threadIdx.x & (B - 1);
    const long long row = (long long)blockIdx.x * (256 / B) + (threadIdx.x / B);
    if (row >= N) return;                                      // (the whole group)
    long long e0 = rowptr[row], e1 = rowptr[row + 1];
    e0 = e0 < 0 ? 0 : e0;
    e1 = e1 > nnz ? nnz : e1;
    double acc = 0.0;
    for (long long base = e0; base < e1; base += B) {
        const long long me = base + l;
        int jm = -1;                                           // (-1: no entry, or a column outside [0, N): nothing is read for it)
        double cm = 0.0;
        if (me < e1) {
            const long long j = col[me];
            if (j >= 0 && j < N) {
                jm = (int)j;
                cm = (double)val[me] * scale[j];
            }
        }
        const int cnt = (int)((e1 - base) < (long long)B ? (e1 - base) : (long long)B);      // (the same in every lane of the group)
        for (int u0 = 0; u0 < cnt; u0 += SP_DEPTH) {
            double c[SP_DEPTH], x[SP_DEPTH];
            int jj[SP_DEPTH];
#pragma unroll
            for (int u = 0; u < SP_DEPTH; ++u) {
                jj[u] = __shfl(jm, u0 + u, B);
                c[u] = __shfl(cm, u0 + u, B);
                if (u0 + u >= cnt) jj[u] = -1;
                x[u] = 0.0;
                if (jj[u] >= 0) x[u] = in[(long long)jj[u] * B + l];
            }
#pragma unroll
            for (int u = 0; u < SP_DEPTH; ++u)                  // added in entry order
                if (jj[u] >= 0) acc = acc + c[u] * x[u];
        }
    }
    const long long at = row * B + l;
    double r = (alpha * scale[row]) * acc + gamma * in[at];
    if (prev) r = r - beta * prev[at];                         // (read by its one owner before `out`, which may be `prev`, is written)
    out[at] = r;
}

// ---- Gram matrix of two blocks ----
// Workgroup s takes rows [512 s, 512 s + 512) in tiles of 64 rows staged in LDS; thread t owns elements t, t + 256, ... of the
// B x B result, (a, b) = (element / B, element % B), and adds fma(Y[r, a], Z[r, b], acc) over the rows in ascending order (rows
// past N are zeros).  part[s] is the segment's B x B sum.
template <int B>
__global__ __launch_bounds__(256) void spectral_gram_kernel(const double* __restrict__ Y, const double* __restrict__ Z, long long N,
                                                            double* __restrict__ part) {
    __shared__ double Ys[SP_GRAM_TILE * B];
    __shared__ double Zs[SP_GRAM_TILE * B];
    constexpr int OWN = B * B / 256;
    const bool same = Y == Z;
    const double* zs = same ? Ys : Zs;
    const long long r0 = (long long)blockIdx.x * SP_GRAM_ROWS;
    double acc[OWN];
#pragma unroll
    for (int m = 0; m < OWN; ++m) acc[m] = 0.0;
    for (int t0 = 0; t0 < SP_GRAM_ROWS; t0 += SP_GRAM_TILE) {
        const long long base = (r0 + t0) * B, end = N * B;
        if (r0 + t0 >= N) break;                               // (the whole workgroup)
        for (int q = threadIdx.x; q < SP_GRAM_TILE * B; q += 256) {
            const long long at = base + q;
            Ys[q] = at < end ? Y[at] : 0.0;
            if (!same) Zs[q] = at < end ? Z[at] : 0.0;
        }
        __syncthreads();
#pragma unroll 4
        for (int r = 0; r < SP_GRAM_TILE; ++r) {
#pragma unroll
            for (int m = 0; m < OWN; ++m) {
                const int el = threadIdx.x + 256 * m;
                acc[m] = __builtin_fma(Ys[r * B + el / B], zs[r * B + el % B], acc[m]);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int m = 0; m < OWN; ++m) part[(long long)blockIdx.x * (B * B) + threadIdx.x + 256 * m] = acc[m];
}

// one workgroup: element q of the result = part[0][q] + part[1][q] + ... in segment order
__global__ __launch_bounds__(256) void spectral_gram_sum_kernel(const double* __restrict__ part, long long segments, int BB,
                                                                double* __restrict__ out) {
#pragma clang fp contract(off)
    for (int q = threadIdx.x; q < BB; q += 256) {
        double acc = 0.0;
        for (long long s = 0; s < segments; ++s) acc = acc + part[s * BB + q];
        out[q] = acc;
    }
}

// ---- out = Y1 M1 (+ Y2 M2) ----
// A workgroup takes 256 / B rows; the rows of Y1 (Y2) and the matrices are staged in LDS.  The thread of (row, l):
//   a1 = fma(Y1[row, c], M1[c, l], a1) for c = 0 .. B - 1;  a2 likewise;  out = a1 + a2   (out = a1 without Y2).
template <int B>
__global__ __launch_bounds__(256) void spectral_rotate_kernel(const double* __restrict__ Y1, const double* __restrict__ M1,
                                                              const double* __restrict__ Y2, const double* __restrict__ M2,
                                                              long long N, double* __restrict__ out) {
    __shared__ double Ms1[B * B];
    __shared__ double Ms2[B * B];
    __shared__ double Rs1[256];
    __shared__ double Rs2[256];
    const bool two = Y2 != nullptr;
    for (int q = threadIdx.x; q < B * B; q += 256) {
        Ms1[q] = M1[q];
        if (two) Ms2[q] = M2[q];
    }
    const long long at = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool live = at < N * B;
    Rs1[threadIdx.x] = live ? Y1[at] : 0.0;
    if (two) Rs2[threadIdx.x] = live ? Y2[at] : 0.0;
    __syncthreads();
    const int l = threadIdx.x & (B - 1), g = threadIdx.x & ~(B - 1);
    double a1 = 0.0, a2 = 0.0;
#pragma unroll
    for (int c = 0; c < B; ++c) a1 = __builtin_fma(Rs1[g + c], Ms1[c * B + l], a1);
    if (two) {
#pragma unroll
        for (int c = 0; c < B; ++c) a2 = __builtin_fma(Rs2[g + c], Ms2[c * B + l], a2);
        a1 = a1 + a2;
    }
    if (live) out[at] = a1;
}

inline bool sp_width(int B) { return B == 16 || B == 32; }

}  // namespace

extern "C" int jamie_graph_rowsum(const long long* rowptr, const int32_t* col, const float* val, const double* w, long long N,
                                  long long nnz, double* out, void* stream) {
    JAMIE_ARG(rowptr && col && val && out, "null pointer");
    JAMIE_ARG(N >= 1 && N < 2147483647ll && nnz >= 0, "1 <= N < 2^31, nnz >= 0");
    JAMIE_ARG(out != w, "out and w must be two buffers");
    const long long blocks = (N + 256 / SP_GROUP - 1) / (256 / SP_GROUP);
    hipLaunchKernelGGL(spectral_rowsum_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, rowptr, col, val, w, N, nnz,
                       out);
    return jamie_launch_status("jamie_graph_rowsum");
}

extern "C" int jamie_graph_cheb_step(const long long* rowptr, const int32_t* col, const float* val, long long nnz, const double* scale,
                                     const double* in, const double* prev, double* out, long long N, int B, double alpha,
                                     double gamma, double beta, void* stream) {
    JAMIE_ARG(rowptr && col && val && scale && in && out, "null pointer");
    JAMIE_ARG(sp_width(B), "B is 16 or 32");
    JAMIE_ARG(N >= 1 && N < 2147483647ll && nnz >= 0, "1 <= N < 2^31, nnz >= 0");
    JAMIE_ARG(out != in && prev != in, "in must differ from out and prev");
    JAMIE_ARG((const void*)out != (const void*)scale, "out and scale must be two buffers");
    JAMIE_ARG(alpha == alpha && gamma == gamma && beta == beta, "alpha, gamma, beta must be numbers");
    const long long blocks = (N + 256 / B - 1) / (256 / B);
    if (B == 16)
        hipLaunchKernelGGL(spectral_cheb_kernel<16>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, rowptr, col, val, nnz,
                           scale, in, prev, out, N, alpha, gamma, beta);
    else
        hipLaunchKernelGGL(spectral_cheb_kernel<32>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, rowptr, col, val, nnz,
                           scale, in, prev, out, N, alpha, gamma, beta);
    return jamie_launch_status("jamie_graph_cheb_step");
}

extern "C" long long jamie_block_gram_workspace(long long N, int B) {
    if (N < 1 || N >= 2147483647ll || !sp_width(B)) return 0;
    return ((N + SP_GRAM_ROWS - 1) / SP_GRAM_ROWS) * (long long)(B * B) * (long long)sizeof(double);
}

extern "C" int jamie_block_gram(const double* Y, const double* Z, long long N, int B, void* ws, long long ws_bytes, double* out,
                                void* stream) {
    JAMIE_ARG(Y && Z && ws && out, "null pointer");
    JAMIE_ARG(sp_width(B), "B is 16 or 32");
    JAMIE_ARG(N >= 1 && N < 2147483647ll, "1 <= N < 2^31");
    JAMIE_ARG(ws_bytes >= jamie_block_gram_workspace(N, B), "workspace below jamie_block_gram_workspace(N, B)");
    JAMIE_ARG(out != Y && out != Z && (const void*)ws != (const void*)Y && (const void*)ws != (const void*)Z && (void*)out != ws,
              "out and the workspace must differ from the blocks and from one another");
    JAMIE_ARG(((uintptr_t)ws & 7) == 0, "the workspace must be 8-byte aligned");
    const long long segments = (N + SP_GRAM_ROWS - 1) / SP_GRAM_ROWS;
    if (B == 16)
        hipLaunchKernelGGL(spectral_gram_kernel<16>, dim3((unsigned)segments), dim3(256), 0, (hipStream_t)stream, Y, Z, N, (double*)ws);
    else
        hipLaunchKernelGGL(spectral_gram_kernel<32>, dim3((unsigned)segments), dim3(256), 0, (hipStream_t)stream, Y, Z, N, (double*)ws);
    const int rc = jamie_launch_status("jamie_block_gram");
    if (rc) return rc;
    hipLaunchKernelGGL(spectral_gram_sum_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)ws, segments, B * B, out);
    return jamie_launch_status("jamie_block_gram");
}

extern "C" int jamie_block_rotate(const double* Y1, const double* M1, const double* Y2, const double* M2, long long N, int B,
                                  double* out, void* stream) {
    JAMIE_ARG(Y1 && M1 && out, "null pointer");
    JAMIE_ARG((Y2 == nullptr) == (M2 == nullptr), "Y2 and M2 are given together");
    JAMIE_ARG(sp_width(B), "B is 16 or 32");
    JAMIE_ARG(N >= 1 && N < 2147483647ll, "1 <= N < 2^31");
    JAMIE_ARG(out != Y1 && out != Y2 && out != M1 && out != M2, "out must differ from the inputs");
    const long long blocks = (N * B + 255) / 256;
    if (B == 16)
        hipLaunchKernelGGL(spectral_rotate_kernel<16>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, Y1, M1, Y2, M2, N, out);
    else
        hipLaunchKernelGGL(spectral_rotate_kernel<32>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, Y1, M1, Y2, M2, N, out);
    return jamie_launch_status("jamie_block_rotate");
}

// Imputation metrics on the device (include/jamie_hip.h "Imputation metrics on the device"; jamie_amd/imputation.py): per-feature
// Pearson correlation, mean squared error and AUROC between an imputed and a measured [N, d] fp32 matrix.
//
// Moments (jamie_feature_stats): one pass over both matrices.  Every element is widened to fp64 and shifted by its feature's
// pivot (row 0's value) in fp64; the six sums per feature -- dx, dy, dx^2, dy^2, dx dy, (x - y)^2 -- are kept in fp64.  A
// workgroup owns 64 features x ROWB rows (16 lanes x float4 across the features, 16 row groups, 4 rows of both matrices in flight
// per thread), adds its 16 row groups in order and writes fp64 partials; the finalise kernel adds the row blocks in order.  No
// float atomics: every bit of the result is the same from run to run.  A constant column has dx = 0 in every row, its sum of
// squares is exactly 0, and its r is NaN by that test.
//
// AUROC (jamie_feature_auroc): label Y > thr, score X.  The negatives' scores of a group of features are sorted feature-major as
// order-preserving uint32 keys (positives and padding: the sentinel 0xFFFFFFFF, past every finite score): a tile transpose, a
// bitonic sort of CHUNK keys per workgroup in LDS, then rank-merge passes between two buffers until a feature is one run (merge-path
// windows, ranked in LDS).  Every
// positive then finds how many negatives are below it and how many tie with it by two binary searches.  U2 = sum over positives
// of (2 #below + #tied) and n_pos are integers added with integer atomics: exact and order-independent.
#include "common.h"
#include "key_sort.h"

namespace {

constexpr int ROWB = 512;              // rows of a stats workgroup (jamie_amd/imputation.py ROW_BLOCK)
constexpr int NRG = 16;                // row groups of a stats workgroup
constexpr int NQ = 6;                  // sums per feature
constexpr int MAX_GROUP = 32768;       // features per jamie_feature_auroc call (a grid dimension)

// columns [col, col + 4) of a row; 0 where the column does not exist
__device__ __forceinline__ float4 load4(const float* __restrict__ p, int col, int d, bool vec) {
    if (vec) return *reinterpret_cast<const float4*>(p);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    v.x = p[0];
    if (col + 1 < d) v.y = p[1];
    if (col + 2 < d) v.z = p[2];
    if (col + 3 < d) v.w = p[3];
    return v;
}

__device__ __forceinline__ void stats_add(double (&acc)[NQ][4], const float4& x, const float4& y, const double (&px)[4],
                                          const double (&py)[4]) {
    const float xs[4] = {x.x, x.y, x.z, x.w}, ys[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double xd = (double)xs[k], yd = (double)ys[k];
        const double dx = xd - px[k], dy = yd - py[k], e = xd - yd;
        acc[0][k] += dx;
        acc[1][k] += dy;
        acc[2][k] += dx * dx;
        acc[3][k] += dy * dy;
        acc[4][k] += dx * dy;
        acc[5][k] += e * e;
    }
}

// part[(rb * NQ + q) * d + f]: the sums of row block rb
__global__ __launch_bounds__(256) void feature_stats_kernel(const float* __restrict__ X, const float* __restrict__ Y, long long N,
                                                            int d, int vec, double* __restrict__ part) {
    __shared__ double sh[NRG][64];
    const int c4 = threadIdx.x & 15, rg = threadIdx.x >> 4;
    const int col = blockIdx.x * 64 + c4 * 4;
    const long long r0 = (long long)blockIdx.y * ROWB;
    const long long r1 = r0 + ROWB < N ? r0 + ROWB : N;
    double acc[NQ][4];
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[q][k] = 0.0;
    if (col < d) {
        const bool v = vec != 0 && col + 3 < d;
        const float4 x0 = load4(X + col, col, d, v), y0 = load4(Y + col, col, d, v);
        const double px[4] = {(double)x0.x, (double)x0.y, (double)x0.z, (double)x0.w};
        const double py[4] = {(double)y0.x, (double)y0.y, (double)y0.z, (double)y0.w};
        long long m = r0 + rg;
        for (; m + 3 * NRG < r1; m += 4 * NRG) {
            float4 x[4], y[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                x[u] = load4(X + (m + NRG * u) * d + col, col, d, v);
                y[u] = load4(Y + (m + NRG * u) * d + col, col, d, v);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) stats_add(acc, x[u], y[u], px, py);
        }
        for (; m < r1; m += NRG) {
            const float4 x = load4(X + m * d + col, col, d, v), y = load4(Y + m * d + col, col, d, v);
            stats_add(acc, x, y, px, py);
        }
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k) sh[rg][c4 * 4 + k] = acc[q][k];
        __syncthreads();
        if (threadIdx.x < 64) {
            const int oc = blockIdx.x * 64 + threadIdx.x;
            if (oc < d) {
                double t = 0.0;
                for (int i = 0; i < NRG; ++i) t += sh[i][threadIdx.x];
                part[((long long)blockIdx.y * NQ + q) * d + oc] = t;
            }
        }
    }
}

// 8 features per workgroup, the row blocks dealt to 32 slices (slice s adds blocks s, s + 32, ... in order), the slices added in order
constexpr int FIN_F = 8, FIN_S = 32;
__global__ __launch_bounds__(256) void feature_stats_final_kernel(const double* __restrict__ part, long long N, int d, int nrb,
                                                                  double* __restrict__ r, double* __restrict__ mse) {
    __shared__ double sh[NQ][FIN_S][FIN_F];
    const int c = threadIdx.x % FIN_F, sl = threadIdx.x / FIN_F;
    const int f = blockIdx.x * FIN_F + c;
    double s[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) s[q] = 0.0;
    if (f < d)
        for (int rb = sl; rb < nrb; rb += FIN_S)
#pragma unroll
            for (int q = 0; q < NQ; ++q) s[q] += part[((long long)rb * NQ + q) * d + f];
#pragma unroll
    for (int q = 0; q < NQ; ++q) sh[q][sl][c] = s[q];
    __syncthreads();
    if (sl != 0 || f >= d) return;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        double t = 0.0;
        for (int i = 0; i < FIN_S; ++i) t += sh[q][i][c];
        s[q] = t;
    }
    const double n = (double)N;
    const double vx = s[2] - s[0] * s[0] / n, vy = s[3] - s[1] * s[1] / n, cov = s[4] - s[0] * s[1] / n;
    // (a sum of squares of fp32 differences is 0 only when every difference is: no underflow in fp64)
    r[f] = (s[2] == 0.0 || s[3] == 0.0) ? __builtin_nan("") : cov / (sqrt(vx) * sqrt(vy));
    mse[f] = s[5] / n;
}

// ---- AUROC (key map, searches, chunk sort and merge passes: key_sort.h) ----
// A 64 rows x 64 features tile of the scores, read along the features and handed on along the rows: a wave then holds 64
// consecutive cells of one feature.  A workgroup walks `tiles` consecutive row tiles and keeps its sums in registers: one integer
// atomic per feature and workgroup.  COUNT = false: the key pass, keys[c][i] = key of a negative, the sentinel for a positive or a
// padding row, and n_pos.  COUNT = true: every positive is ranked in the sorted negatives keys[c][0, n_neg) of its feature.
constexpr int MAX_TILES = 8;
template <bool COUNT>
__global__ __launch_bounds__(256) void score_tile_kernel(const float* __restrict__ X, const float* __restrict__ Y, long long N, int d,
                                                         const float* __restrict__ thr, int f0, int dg, long long Npad,
                                                         int tiles, uint32_t* __restrict__ keys, unsigned long long* __restrict__ n_pos,
                                                         unsigned long long* __restrict__ U2) {
    __shared__ uint32_t T[64][65];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c0 = blockIdx.y * 64;
    const long long rows = COUNT ? N : Npad;                   // (the key pass writes the padding too)
    const bool col = c0 + lane < dg;
    const float t = col ? thr[f0 + c0 + lane] : 0.f;
    unsigned long long acc[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[k] = 0;
    for (int tile = 0; tile < tiles; ++tile) {
        const long long i0 = ((long long)blockIdx.x * tiles + tile) * 64;
        if (i0 >= rows) break;                                 // (the same in every thread)
        float x[16], y[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const long long gi = i0 + w + 4 * k;
            const bool in = col && gi < N;
            const long long o = gi * d + f0 + c0 + lane;
            x[k] = in ? X[o] : 0.f;
            y[k] = in ? Y[o] : 0.f;
        }
        if (tile) __syncthreads();                             // the last tile is read
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const bool in = col && i0 + w + 4 * k < N;
            T[w + 4 * k][lane] = (in && (y[k] > t) == COUNT) ? order_key(x[k]) : SENTINEL;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int c = w + 4 * k, gc = c0 + c;
            if (gc < dg) {                                     // (the same in every lane of the wave)
                const uint32_t key = T[lane][c];
                if (!COUNT) {
                    keys[(long long)gc * Npad + i0 + lane] = key;
                    acc[k] += (unsigned long long)__popcll(__ballot(key == SENTINEL && i0 + lane < N));
                } else if (key != SENTINEL) {
                    acc[k] += (unsigned long long)rank2(keys + (long long)gc * Npad, N - (long long)n_pos[f0 + gc], key);
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int gc = c0 + w + 4 * k;
        if (gc < dg) {
            const unsigned long long v = COUNT ? wave_sum_u64(acc[k]) : acc[k];
            if (lane == 0 && v) atomicAdd(COUNT ? &U2[f0 + gc] : &n_pos[f0 + gc], v);
        }
    }
}

// row tiles a workgroup of score_tile_kernel walks: up to 8, fewer while that leaves the device short of workgroups
inline int tiles_per_workgroup(long long rows, unsigned column_tiles) {
    const long long t = (rows + 63) / 64 * column_tiles / 512;
    return t < 1 ? 1 : (t > MAX_TILES ? MAX_TILES : (int)t);
}
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" long long jamie_imputation_workspace(long long N, int d, int which) {
    if (N < 1 || d < 1) return 0;
    if (which == 0) return (N + ROWB - 1) / ROWB * NQ * (long long)d * 8;
    if (which == 1) return 2 * pad_to_chunk(N) * (long long)d * 4;
    return 0;
}

extern "C" int jamie_feature_stats(const float* X, const float* Y, long long N, int d, double* r, double* mse, void* ws,
                                   long long ws_bytes, void* stream) {
    JAMIE_ARG(X && Y && r && mse && ws, "null pointer");
    JAMIE_ARG(N >= 2 && N < 2147483647ll && d >= 1, "2 <= N < 2^31, d >= 1");
    JAMIE_ARG(ws_bytes >= jamie_imputation_workspace(N, d, 0), "workspace smaller than jamie_imputation_workspace(N, d, 0)");
    hipStream_t st = (hipStream_t)stream;
    const int nrb = (int)((N + ROWB - 1) / ROWB);
    JAMIE_ARG(nrb <= 65535, "N <= 65535 * 512");
    const int vec = (d % 4 == 0) && aligned16(X) && aligned16(Y);
    hipLaunchKernelGGL(feature_stats_kernel, dim3((unsigned)((d + 63) / 64), (unsigned)nrb), dim3(256), 0, st, X, Y, N, d, vec,
                       (double*)ws);
    hipLaunchKernelGGL(feature_stats_final_kernel, dim3((unsigned)((d + FIN_F - 1) / FIN_F)), dim3(256), 0, st, (const double*)ws, N, d, nrb,
                       r, mse);
    return jamie_launch_status("jamie_feature_stats");
}

extern "C" int jamie_feature_auroc(const float* X, const float* Y, long long N, int d, const float* thr, int f0, int dg,
                                   long long* n_pos, long long* U2, void* ws, long long ws_bytes, int last_stage, void* stream) {
    JAMIE_ARG(X && Y && thr && n_pos && U2 && ws, "null pointer");
    JAMIE_ARG(N >= 2 && N < 2147483647ll - CHUNK && d >= 1, "2 <= N < 2^31 - CHUNK, d >= 1");
    JAMIE_ARG(f0 >= 0 && dg >= 1 && dg <= MAX_GROUP && f0 + (long long)dg <= d, "0 <= f0, 1 <= dg <= 32768, f0 + dg <= d");
    JAMIE_ARG(ws_bytes >= jamie_imputation_workspace(N, dg, 1), "workspace smaller than jamie_imputation_workspace(N, dg, 1)");
    JAMIE_ARG(((uintptr_t)ws & 15) == 0, "workspace not 16-byte aligned");
    JAMIE_ARG(last_stage >= 1 && last_stage <= 4, "1 <= last_stage <= 4");
    hipStream_t st = (hipStream_t)stream;
    const long long Npad = pad_to_chunk(N);
    uint32_t* a = (uint32_t*)ws;
    uint32_t* b = a + Npad * dg;
    unsigned long long* np = (unsigned long long*)n_pos;
    unsigned long long* u2 = (unsigned long long*)U2;
    if (hipMemsetAsync(n_pos + f0, 0, (size_t)dg * 8, st) != hipSuccess || hipMemsetAsync(U2 + f0, 0, (size_t)dg * 8, st) != hipSuccess)
        return jamie_launch_status("jamie_feature_auroc");
    const unsigned ct = (unsigned)((dg + 63) / 64);
    const int tk = tiles_per_workgroup(Npad, ct), tc = tiles_per_workgroup(N, ct);
    hipLaunchKernelGGL((score_tile_kernel<false>), dim3((unsigned)((Npad + 64 * tk - 1) / (64 * tk)), ct), dim3(256), 0, st, X, Y, N, d,
                       thr, f0, dg, Npad, tk, a, np, u2);
    a = sort_columns(a, b, Npad, dg, last_stage, st);
    if (last_stage >= 4)
        hipLaunchKernelGGL((score_tile_kernel<true>), dim3((unsigned)((N + 64 * tc - 1) / (64 * tc)), ct), dim3(256), 0, st, X, Y, N, d,
                           thr, f0, dg, Npad, tc, a, np, u2);
    return jamie_launch_status("jamie_feature_auroc");
}

// UMAP layout on the device (include/jamie_hip.h "UMAP layout on the device"; jamie_amd/umap.py): the fuzzy neighbour graph on
// the K-neighbour lists of jamie_self_knn and the stochastic layout epochs over its CSR rows.  O(N K) memory.  DESIGN.md §20.
//
//   umap_smooth_knn_kernel   one wave per cell: rho, the bisection of umap-learn's `smooth_knn_dist` for sigma in fp64, the weights
//   umap_mutual_kernel       one thread per (cell, slot): is the cell listed by its neighbour, and a + b - a b of the pair
//   umap_epoch_kernel        16 lanes per row of the graph: which entries fire, their attraction, their negative draws, the move
//
// The CSR rows themselves are written by jamie_tsne_fill.  Deterministic: no floating-point atomics; every sum has one owner and a
// fixed order, and every entry of the schedule has one owner.
#include "lane_tree.h"
#include "mutual.h"

namespace {

constexpr int UM_KMAX = 128;      // neighbours per cell (jamie_self_knn's limit): two per lane of a wave
constexpr int UM_TRIES = 64;      // of the sigma solve
constexpr int UM_GROUP = 16;      // lanes that own a row of the graph in the epoch: a typical row holds 14 .. 30 entries
constexpr int UM_ROWS = 256 / UM_GROUP;      // rows per workgroup
constexpr int UM_NEG_MAX = 64;

// ---- step 1: smooth kNN distances ----
// lane l holds neighbours l and l + 64
__device__ __forceinline__ double umap_psi_sum(double sigma, double e0, double e1, bool have0, bool have1) {
    const double p0 = have0 ? (e0 > 0.0 ? exp(-e0 / sigma) : 1.0) : 0.0;
    const double p1 = have1 ? (e1 > 0.0 ? exp(-e1 / sigma) : 1.0) : 0.0;
    return wave_sum(p0 + p1);
}

__global__ __launch_bounds__(256) void umap_smooth_knn_kernel(const float* __restrict__ dist, long long N, int K, double target,
                                                              double floor_scale, float* __restrict__ W, double* __restrict__ rho_out,
                                                              double* __restrict__ sigma_out, int32_t* __restrict__ tries_out) {
    const int lane = threadIdx.x & 63;
    const long long cell = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (cell >= N) return;                                 // (the whole wave)
    const bool have0 = lane < K, have1 = lane + 64 < K;
    const double D0 = have0 ? (double)dist[cell * K + lane] : 0.0, D1 = have1 ? (double)dist[cell * K + lane + 64] : 0.0;
    const double inf = __builtin_inf();
    // the smallest positive distance of the row (a minimum does not depend on the order it is taken in)
    double rho = fmin(have0 && D0 > 0.0 ? D0 : inf, have1 && D1 > 0.0 ? D1 : inf);
    for (int s = 32; s > 0; s >>= 1) rho = fmin(rho, __shfl_xor(rho, s));
    rho = rho == inf ? 0.0 : rho;
    const double total = wave_sum(D0 + D1);
    const double e0 = D0 - rho, e1 = D1 - rho;
    double lo = 0.0, hi = inf, mid = 1.0;
    int tries = 0;
    while (tries < UM_TRIES) {                             // (the sum is the same bits in every lane: the wave branches as one)
        const double sum = umap_psi_sum(mid, e0, e1, have0, have1);
        ++tries;
        if (fabs(sum - target) < 1e-5) break;
        if (sum > target) {
            hi = mid;
            mid = (lo + hi) / 2.0;
        } else {
            lo = mid;
            mid = hi == inf ? mid * 2.0 : (lo + hi) / 2.0;
        }
    }
    const double floor_sigma = floor_scale * total;
    const double sigma = mid > floor_sigma ? mid : floor_sigma;
    if (have0) W[cell * K + lane] = (e0 <= 0.0 || sigma == 0.0) ? 1.f : (float)exp(-e0 / sigma);
    if (have1) W[cell * K + lane + 64] = (e1 <= 0.0 || sigma == 0.0) ? 1.f : (float)exp(-e1 / sigma);
    if (lane == 0) {
        rho_out[cell] = rho;
        sigma_out[cell] = sigma;
        tries_out[cell] = tries;
    }
}

// ---- step 2: the fuzzy union ----
// (a + b, a b and their difference are taken as doubles: the same bits from either side of the pair)
__global__ __launch_bounds__(256) void umap_mutual_kernel(const int32_t* __restrict__ idx, const float* __restrict__ W, long long N,
                                                          int K, float* __restrict__ val, int32_t* __restrict__ mutual) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= N * K) return;
    const long long i = e / K;
    double other;
    const int m = mutual_search(idx, W, N, K, i, (long long)idx[e], other);
    const double own = (double)W[e];
    val[e] = (float)((own + other) - own * other);
    mutual[e] = m;
}

// ---- steps 4 - 6: one epoch ----
struct UmapCurve {
    float a, b, m2ab, g2b;        // a, b rounded to fp32; -2 a b and 2 gamma b of the ROUNDED a, b, formed in fp64 and rounded once
};

// The coefficient arithmetic is written out operation by operation (no contraction other than the fmas named): the numpy
// restatement of tests/umap_util.py follows it rounding for rounding, up to the power function's own error.
//   d2 = fma(dx, dx, dy dy);  p = powf(d2, b);  q = fma(a, p, 1)
//   attraction: c = (m2ab p) / (d2 q);  repulsion: c = g2b / ((0.001 + d2) q);  each term clip(c dx), clip(c dy)
__device__ __forceinline__ float umap_clip(float v) { return fminf(4.f, fmaxf(-4.f, v)); }

__device__ __forceinline__ void umap_pair(const UmapCurve cv, float dx, float dy, bool attract, float& tx, float& ty) {
#pragma clang fp contract(off)
    const float d2 = __builtin_fmaf(dx, dx, dy * dy);
    if (!(d2 > 0.f)) {
        tx = ty = 0.f;
        return;
    }
    const float p = powf(d2, cv.b);
    const float q = __builtin_fmaf(cv.a, p, 1.f);
    const float c = attract ? (cv.m2ab * p) / (d2 * q) : cv.g2b / ((0.001f + d2) * q);
    tx = umap_clip(c * dx);
    ty = umap_clip(c * dy);
}

// UM_GROUP lanes own row `row`: lane l of the group takes entries l, l + 16, ... of the row.  For each it tests and advances the
// entry's `next` (it is the entry's only owner), and if the entry fires forms s = 2 attraction + draw 0 + draw 1 + ... in fp32 (in
// that order) and adds s to its partial sum.  The group's 16 partial sums are added by the xor tree 8, 4, 2, 1, and lane 0 of the
// group writes y_out = fma(alpha, delta, y_in).
__global__ __launch_bounds__(256) void umap_epoch_kernel(const long long* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                         const float* __restrict__ eps, float* __restrict__ next, long long nnz,
                                                         const float* __restrict__ Yin, float* __restrict__ Yout, long long N,
                                                         int epoch, float alpha, UmapCurve cv, int n_neg, uint32_t seed_lo,
                                                         uint32_t seed_hi, float* __restrict__ delta, int32_t* __restrict__ fired,
                                                         long long* __restrict__ fired_total) {
#pragma clang fp contract(off)
    const int l = threadIdx.x & (UM_GROUP - 1);
    const long long row = (long long)blockIdx.x * UM_ROWS + (threadIdx.x / UM_GROUP);
    const bool live = row < N;
    long long e0 = 0, e1 = 0;
    float xi = 0.f, yi = 0.f;
    if (live) {
        e0 = rowptr[row];
        e1 = rowptr[row + 1];
        e0 = e0 < 0 ? 0 : e0;
        e1 = e1 > nnz ? nnz : e1;
        const float2 v = *reinterpret_cast<const float2*>(Yin + 2 * row);
        xi = v.x;
        yi = v.y;
    }
    const float now = (float)epoch;
    float sx = 0.f, sy = 0.f;
    int count = 0;
    for (long long e = e0 + l; e < e1; e += UM_GROUP) {
        const float nx = next[e];
        if (!(nx <= now)) continue;
        next[e] = nx + eps[e];
        ++count;
        const long long j = col[e];
        if (j < 0 || j >= N) continue;                     // (jamie_umap_epoch's callers check the columns; nothing is read outside Y)
        const float2 yj = *reinterpret_cast<const float2*>(Yin + 2 * j);
        float tx, ty;
        umap_pair(cv, xi - yj.x, yi - yj.y, true, tx, ty);
        float ex = 2.f * tx, ey = 2.f * ty;
        for (int r0 = 0; r0 < n_neg; r0 += 4) {             // the four draws of one Philox block: their gathers are in flight together
            const Philox4 rnd = philox4x32_10((uint32_t)((unsigned long long)e & 0xffffffffull), (uint32_t)((unsigned long long)e >> 32),
                                              (uint32_t)epoch, (uint32_t)(r0 >> 2), seed_lo, seed_hi);
            float2 yk[4];
            bool use[4];
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const long long k = (long long)(((unsigned long long)rnd.v[w] * (unsigned long long)N) >> 32);      // in [0, N)
                use[w] = r0 + w < n_neg && k != row;
                yk[w] = make_float2(0.f, 0.f);
                if (r0 + w < n_neg) yk[w] = *reinterpret_cast<const float2*>(Yin + 2 * k);
            }
#pragma unroll
            for (int w = 0; w < 4; ++w) {                   // added in draw order
                if (!use[w]) continue;
                umap_pair(cv, xi - yk[w].x, yi - yk[w].y, false, tx, ty);
                ex = ex + tx;
                ey = ey + ty;
            }
        }
        sx = sx + ex;
        sy = sy + ey;
    }
    for (int s = UM_GROUP / 2; s > 0; s >>= 1) {           // (every lane of the wave is here: no lane has left)
        sx = sx + __shfl_xor(sx, s);
        sy = sy + __shfl_xor(sy, s);
        count += __shfl_xor(count, s);
    }
    if (live && l == 0) {
        float2 out;
        out.x = __builtin_fmaf(alpha, sx, xi);
        out.y = __builtin_fmaf(alpha, sy, yi);
        *reinterpret_cast<float2*>(Yout + 2 * row) = out;
        if (delta) {
            delta[2 * row] = sx;
            delta[2 * row + 1] = sy;
        }
        if (fired) fired[row] = count;
        if (fired_total) fired_total[row] += (long long)count;
    }
}

}  // namespace

extern "C" int jamie_umap_smooth_knn(const float* dist, long long N, int K, int n_neighbors, double target, float* W, double* rho,
                                     double* sigma, int32_t* tries, void* stream) {
    JAMIE_ARG(dist && W && rho && sigma && tries, "null pointer");
    JAMIE_ARG(N >= 1 && K >= 1 && K <= UM_KMAX, "N >= 1, 1 <= K <= 128");
    JAMIE_ARG(n_neighbors >= 2 && target > 0.0 && target < 1e300, "n_neighbors >= 2, a finite positive target");
    JAMIE_ARG((N + 3) / 4 <= 2147483647ll, "N too large for one launch");
    hipLaunchKernelGGL(umap_smooth_knn_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, (hipStream_t)stream, dist, N, K, target,
                       1e-3 / (double)n_neighbors, W, rho, sigma, tries);
    return jamie_launch_status("jamie_umap_smooth_knn");
}

extern "C" int jamie_umap_mutual(const int32_t* idx, const float* W, long long N, int K, float* val, int32_t* mutual, void* stream) {
    JAMIE_ARG(idx && W && val && mutual, "null pointer");
    JAMIE_ARG(N >= 1 && N < 2147483647ll && K >= 1 && K <= UM_KMAX, "1 <= N < 2^31, 1 <= K <= 128");
    const long long blocks = (N * K + 255) / 256;
    JAMIE_ARG(blocks <= 2147483647ll, "N K too large for one launch");
    hipLaunchKernelGGL(umap_mutual_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, idx, W, N, K, val, mutual);
    return jamie_launch_status("jamie_umap_mutual");
}

extern "C" int jamie_umap_epoch(const long long* rowptr, const int32_t* col, const float* eps, float* next, long long nnz,
                                const float* Y_in, float* Y_out, long long N, int epoch, double alpha, double a, double b,
                                double gamma, int negative_sample_rate, unsigned long long seed, float* delta, int32_t* fired,
                                long long* fired_total, void* stream) {
    JAMIE_ARG(rowptr && col && eps && next && Y_in && Y_out, "null pointer");
    JAMIE_ARG(Y_in != Y_out, "Y_in and Y_out must be two buffers");
    JAMIE_ARG(N >= 2 && N < 2147483647ll && nnz >= 0 && epoch >= 0, "2 <= N < 2^31, nnz >= 0, epoch >= 0");
    JAMIE_ARG(a > 0.0 && b > 0.0 && a < 1e30 && b < 1e30, "a and b must be positive");
    JAMIE_ARG(gamma > 0.0 && gamma < 1e30 && alpha >= 0.0 && alpha < 1e30, "gamma positive, alpha not negative");
    JAMIE_ARG(negative_sample_rate >= 1 && negative_sample_rate <= UM_NEG_MAX, "1 <= negative_sample_rate <= 64");
    JAMIE_ARG((((uintptr_t)Y_in | (uintptr_t)Y_out) & 7) == 0, "Y_in and Y_out must be 8-byte aligned");
    UmapCurve cv;
    cv.a = (float)a;
    cv.b = (float)b;
    cv.m2ab = (float)(-2.0 * (double)cv.a * (double)cv.b);      // (of the rounded a, b: the curve both routes use)
    cv.g2b = (float)(2.0 * gamma * (double)cv.b);
    const long long blocks = (N + UM_ROWS - 1) / UM_ROWS;
    hipLaunchKernelGGL(umap_epoch_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, rowptr, col, eps, next, nnz, Y_in,
                       Y_out, N, epoch, (float)alpha, cv, negative_sample_rate, (uint32_t)(seed & 0xffffffffull),
                       (uint32_t)(seed >> 32), delta, fired, fired_total);
    return jamie_launch_status("jamie_umap_epoch");
}

// Marker features per group on the device (include/jamie_hip.h "Marker features on the device"; jamie_amd/markers.py): for an
// [N, d] fp32 matrix of cells x features and a group code per cell, the exact one-vs-rest rank sums of every (feature, group) and
// the fp64 moments of every (group, feature).
//
// The cells are visited in group order: the host passes a stable argsort of the codes (`order`), the sorted codes and the segment
// offsets.  X itself is not permuted or copied, the number of groups is unbounded and no per-group table lives in LDS.
//
// Rank sums (jamie_group_rank_sums): every cell's value of a group of features becomes an order-preserving uint32 key, the columns
// are sorted feature-major (key_sort.h: LDS chunk sort + rank-merge passes), and every cell then finds lb = #{keys below its own}
// and ub = #{keys not above it} in its feature's sorted column by two binary searches side by side.  lb + ub + 1 is twice its
// midrank and (ub - lb)^2 - 1, summed over the cells, is the tie term sum (t^3 - t): a tie group of t cells gives t (t^2 - 1).  A wave
// holds 64 group-sorted cells of one feature, adds the runs of equal code by a segmented scan and issues one integer atomic per
// run: integer sums are exact in any order, so every bit is the same from run to run.
//
// Moments (jamie_group_moments): the fp64 sum and sum of squares of x - x[0, feature] per (group, feature).  A workgroup takes 64
// features and a piece of at most PIECE consecutive cells of one group's segment (16 lanes x float4 across the features, 16 row
// groups that each add their rows in order, then the row groups in order); a second kernel adds a group's pieces in ascending
// order.  No floating-point atomics.
#include "common.h"
#include "key_sort.h"

namespace {

constexpr int PIECE = 512;             // cells of a moments workgroup (jamie_amd/markers.py PIECE)
constexpr int NRG = 16;                // row groups of a moments workgroup
constexpr int MAX_GROUP = 32768;       // features per jamie_group_rank_sums call (a grid dimension)
constexpr long long MAX_CELLS = 1ll << 21;   // N^3 - N, the tie term of a constant feature, stays below 2^63; twice a rank below 2^32
constexpr int MAX_TILES = 8;

// lb = lower_bound(key), ub = lower_bound(key + 1) in the sorted a[0, n), key below the sentinel: rank2's loop, both results kept
__device__ __forceinline__ void rank_pair(const uint32_t* __restrict__ a, long long n, uint32_t key, long long& lb, long long& ub) {
    long long b0 = 0, b1 = 0;
    const uint32_t k1 = key + 1;
    while (n > 1) {
        const long long half = n >> 1;
        const uint32_t v0 = a[b0 + half - 1], v1 = a[b1 + half - 1];
        b0 += v0 < key ? half : 0;
        b1 += v1 < k1 ? half : 0;
        n -= half;
    }
    if (n == 1) {
        const uint32_t v0 = a[b0], v1 = a[b1];
        b0 += v0 < key ? 1 : 0;
        b1 += v1 < k1 ? 1 : 0;
    }
    lb = b0;
    ub = b1;
}

// The key pass: a 64 cells x 64 features tile, read along the features and written along the cells.  keys[c][i] = key of cell i,
// the sentinel for the padding rows [N, Npad).
__global__ __launch_bounds__(256) void group_key_kernel(const float* __restrict__ X, long long N, int d, int f0, int dg, long long Npad,
                                                        int tiles, uint32_t* __restrict__ keys) {
    __shared__ uint32_t T[64][65];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c0 = blockIdx.y * 64;
    const bool col = c0 + lane < dg;
    for (int tile = 0; tile < tiles; ++tile) {
        const long long i0 = ((long long)blockIdx.x * tiles + tile) * 64;
        if (i0 >= Npad) break;                                 // (the same in every thread)
        float x[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const long long gi = i0 + w + 4 * k;
            x[k] = (col && gi < N) ? X[gi * d + f0 + c0 + lane] : 0.f;
        }
        if (tile) __syncthreads();                             // the last tile is read
#pragma unroll
        for (int k = 0; k < 16; ++k) T[w + 4 * k][lane] = (col && i0 + w + 4 * k < N) ? order_key(x[k]) : SENTINEL;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int c = w + 4 * k, gc = c0 + c;
            if (gc < dg) keys[(long long)gc * Npad + i0 + lane] = T[lane][c];      // (Npad is a multiple of 64)
        }
    }
}

// The ranking pass: tiles of 64 group-sorted cells (rows gathered through `order`) x 64 features.  A wave holds 64 cells of one
// feature with ascending codes: R2[feature][group] += lb + ub + 1 per cell, one atomic per run of equal code; tie[feature] +=
// (ub - lb)^2 - 1, kept in registers over the workgroup's tiles.  A code outside [0, G) or a row outside [0, N) adds nothing.
__global__ __launch_bounds__(256) void group_rank_kernel(const float* __restrict__ X, long long N, int d, const int32_t* __restrict__ order,
                                                         const int32_t* __restrict__ codes, int G, int f0, int dg, long long Npad,
                                                         int tiles, const uint32_t* __restrict__ keys, unsigned long long* __restrict__ R2,
                                                         unsigned long long* __restrict__ tie) {
    __shared__ uint32_t T[64][65];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c0 = blockIdx.y * 64;
    const bool col = c0 + lane < dg;
    unsigned long long tacc[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) tacc[k] = 0;
    for (int tile = 0; tile < tiles; ++tile) {
        const long long i0 = ((long long)blockIdx.x * tiles + tile) * 64;
        if (i0 >= N) break;                                    // (the same in every thread)
        float x[16];
        bool in[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const long long p = i0 + w + 4 * k;
            const long long row = p < N ? (long long)order[p] : -1;
            in[k] = col && row >= 0 && row < N;
            x[k] = in[k] ? X[row * d + f0 + c0 + lane] : 0.f;
        }
        if (tile) __syncthreads();                             // the last tile is read
#pragma unroll
        for (int k = 0; k < 16; ++k) T[w + 4 * k][lane] = in[k] ? order_key(x[k]) : SENTINEL;
        __syncthreads();
        int code = i0 + lane < N ? codes[i0 + lane] : -1;
        if (code >= G) code = -1;
        const int next = __shfl_down(code, 1);
        const bool last = lane == 63 || next != code;          // the lane that ends a run of equal code
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int c = w + 4 * k, gc = c0 + c;
            if (gc < dg) {                                     // (the same in every lane of the wave)
                const uint32_t key = T[lane][c];
                unsigned long long v = 0;
                if (key != SENTINEL && code >= 0) {
                    long long lb, ub;
                    rank_pair(keys + (long long)gc * Npad, N, key, lb, ub);
                    v = (unsigned long long)(lb + ub + 1);
                    const unsigned long long t = (unsigned long long)(ub - lb);
                    tacc[k] += t * t - 1;
                }
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {             // inclusive scan within the runs: the codes ascend, so an equal
                    const unsigned long long u = __shfl_up(v, o);      // code o lanes down means one run in between
                    const int cu = __shfl_up(code, o);
                    if (lane >= o && cu == code) v += u;
                }
                if (last && code >= 0 && v) atomicAdd(&R2[(long long)(f0 + gc) * G + code], v);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int gc = c0 + w + 4 * k;
        if (gc < dg) {
            const unsigned long long v = wave_sum_u64(tacc[k]);
            if (lane == 0 && v) atomicAdd(&tie[f0 + gc], v);
        }
    }
}

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

__device__ __forceinline__ void moments_add(double (&acc)[2][4], const float4& x, const double (&px)[4]) {
    const float xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double dx = (double)xs[k] - px[k];
        acc[0][k] += dx;
        acc[1][k] += dx * dx;
    }
}

// part[(piece * d + f) * 2 + q]: the sums of piece blockIdx.x, which belongs to the last group g with piece_off[g] <= piece
__global__ __launch_bounds__(256) void group_moments_kernel(const float* __restrict__ X, long long N, int d, int vec,
                                                            const int32_t* __restrict__ order, const int32_t* __restrict__ seg_off,
                                                            const int32_t* __restrict__ piece_off, int G, double* __restrict__ part) {
    __shared__ double sh[NRG][64];
    const int c4 = threadIdx.x & 15, rg = threadIdx.x >> 4;
    const int col = blockIdx.y * 64 + c4 * 4;
    const int b = (int)blockIdx.x;
    int g = 0, hi = G;
    while (hi - g > 1) {                                       // (the same in every thread)
        const int mid = (g + hi) >> 1;
        if (piece_off[mid] <= b) g = mid; else hi = mid;
    }
    long long r0 = (long long)seg_off[g] + (long long)(b - piece_off[g]) * PIECE, r1 = seg_off[g + 1];
    if (r0 < 0) r0 = 0;
    if (r1 > r0 + PIECE) r1 = r0 + PIECE;
    if (r1 > N) r1 = N;
    double acc[2][4];
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[q][k] = 0.0;
    if (col < d) {
        const bool v = vec != 0 && col + 3 < d;
        const float4 x0 = load4(X + col, col, d, v);
        const double px[4] = {(double)x0.x, (double)x0.y, (double)x0.z, (double)x0.w};
        long long m = r0 + rg;
        for (; m + 3 * NRG < r1; m += 4 * NRG) {
            float4 x[4];
            bool in[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const long long row = order[m + NRG * u];
                in[u] = row >= 0 && row < N;
                x[u] = load4(X + (in[u] ? row : 0) * d + col, col, d, v);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (in[u]) moments_add(acc, x[u], px);
        }
        for (; m < r1; m += NRG) {
            const long long row = order[m];
            if (row >= 0 && row < N) moments_add(acc, load4(X + row * d + col, col, d, v), px);
        }
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k) sh[rg][c4 * 4 + k] = acc[q][k];
        __syncthreads();
        if (threadIdx.x < 64) {
            const int oc = blockIdx.y * 64 + threadIdx.x;
            if (oc < d) {
                double t = 0.0;
                for (int i = 0; i < NRG; ++i) t += sh[i][threadIdx.x];
                part[((long long)b * d + oc) * 2 + q] = t;
            }
        }
    }
}

// sums[(g * d + f) * 2 + q]: the pieces of group blockIdx.x added in ascending order
__global__ __launch_bounds__(256) void group_moments_final_kernel(const double* __restrict__ part, int d, const int32_t* __restrict__ piece_off,
                                                                  long long n_pieces, double* __restrict__ sums) {
    const int g = (int)blockIdx.x;
    const int f = blockIdx.y * 256 + threadIdx.x;
    if (f >= d) return;
    long long p0 = piece_off[g], p1 = piece_off[g + 1];
    if (p0 < 0) p0 = 0;
    if (p1 > n_pieces) p1 = n_pieces;
    double s0 = 0.0, s1 = 0.0;
    for (long long p = p0; p < p1; ++p) {
        const double2 v = *reinterpret_cast<const double2*>(part + (p * d + f) * 2);
        s0 += v.x;
        s1 += v.y;
    }
    *reinterpret_cast<double2*>(sums + ((long long)g * d + f) * 2) = make_double2(s0, s1);
}

// row tiles a workgroup of the tile kernels walks: up to 8, fewer while that leaves the device short of workgroups
inline int tiles_per_workgroup(long long rows, unsigned column_tiles) {
    const long long t = (rows + 63) / 64 * column_tiles / 512;
    return t < 1 ? 1 : (t > MAX_TILES ? MAX_TILES : (int)t);
}
inline long long max_pieces(long long N, int G) { return N / PIECE + G; }      // sum over the groups of ceil(n_g / PIECE) <= this

}  // namespace

extern "C" long long jamie_markers_workspace(long long N, int d, int G, int which) {
    if (N < 1 || N > MAX_CELLS || d < 1 || G < 1) return 0;
    if (which == 0) return max_pieces(N, G) * (long long)d * 16;
    if (which == 1) return 2 * pad_to_chunk(N) * (long long)d * 4;
    return 0;
}

extern "C" int jamie_group_rank_sums(const float* X, long long N, int d, const int32_t* order, const int32_t* codes, int G, int f0,
                                     int dg, long long* R2, long long* tie, void* ws, long long ws_bytes, int last_stage,
                                     void* stream) {
    JAMIE_ARG(X && order && codes && R2 && tie && ws, "null pointer");
    JAMIE_ARG(N >= 2 && N <= MAX_CELLS && d >= 1 && G >= 1, "2 <= N <= 2^21, d >= 1, G >= 1");
    JAMIE_ARG(f0 >= 0 && dg >= 1 && dg <= MAX_GROUP && f0 + (long long)dg <= d, "0 <= f0, 1 <= dg <= 32768, f0 + dg <= d");
    JAMIE_ARG(ws_bytes >= jamie_markers_workspace(N, dg, G, 1), "workspace smaller than jamie_markers_workspace(N, dg, G, 1)");
    JAMIE_ARG(((uintptr_t)ws & 15) == 0, "workspace not 16-byte aligned");
    JAMIE_ARG(last_stage >= 1 && last_stage <= 4, "1 <= last_stage <= 4");
    hipStream_t st = (hipStream_t)stream;
    const long long Npad = pad_to_chunk(N);
    uint32_t* a = (uint32_t*)ws;
    uint32_t* b = a + Npad * dg;
    if (hipMemsetAsync(R2 + (long long)f0 * G, 0, (size_t)dg * G * 8, st) != hipSuccess ||
        hipMemsetAsync(tie + f0, 0, (size_t)dg * 8, st) != hipSuccess)
        return jamie_launch_status("jamie_group_rank_sums");
    const unsigned ct = (unsigned)((dg + 63) / 64);
    const int tk = tiles_per_workgroup(Npad, ct), tc = tiles_per_workgroup(N, ct);
    hipLaunchKernelGGL(group_key_kernel, dim3((unsigned)((Npad + 64 * tk - 1) / (64 * tk)), ct), dim3(256), 0, st, X, N, d, f0, dg, Npad,
                       tk, a);
    a = sort_columns(a, b, Npad, dg, last_stage, st);
    if (last_stage >= 4)
        hipLaunchKernelGGL(group_rank_kernel, dim3((unsigned)((N + 64 * tc - 1) / (64 * tc)), ct), dim3(256), 0, st, X, N, d, order, codes,
                           G, f0, dg, Npad, tc, a, (unsigned long long*)R2, (unsigned long long*)tie);
    return jamie_launch_status("jamie_group_rank_sums");
}

extern "C" int jamie_group_moments(const float* X, long long N, int d, const int32_t* order, const int32_t* seg_off,
                                   const int32_t* piece_off, int G, long long n_pieces, double* sums, void* ws, long long ws_bytes,
                                   void* stream) {
    JAMIE_ARG(X && order && seg_off && piece_off && sums && ws, "null pointer");
    JAMIE_ARG(N >= 2 && N <= MAX_CELLS && d >= 1 && G >= 1, "2 <= N <= 2^21, d >= 1, G >= 1");
    JAMIE_ARG((d + 63) / 64 <= 65535, "d <= 65535 * 64");
    JAMIE_ARG(n_pieces >= 1 && n_pieces <= max_pieces(N, G), "1 <= n_pieces <= N / 512 + G");
    JAMIE_ARG(ws_bytes >= jamie_markers_workspace(N, d, G, 0), "workspace smaller than jamie_markers_workspace(N, d, G, 0)");
    JAMIE_ARG(((uintptr_t)ws & 15) == 0 && ((uintptr_t)sums & 15) == 0, "workspace or sums not 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int vec = (d % 4 == 0) && ((uintptr_t)X & 15) == 0;
    hipLaunchKernelGGL(group_moments_kernel, dim3((unsigned)n_pieces, (unsigned)((d + 63) / 64)), dim3(256), 0, st, X, N, d, vec, order,
                       seg_off, piece_off, G, (double*)ws);
    hipLaunchKernelGGL(group_moments_final_kernel, dim3((unsigned)G, (unsigned)((d + 255) / 256)), dim3(256), 0, st, (const double*)ws, d,
                       piece_off, n_pieces, sums);
    return jamie_launch_status("jamie_group_moments");
}

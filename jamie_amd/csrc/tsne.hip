// Layout on the device (include/jamie_hip.h "Layout on the device"; jamie_amd/tsne.py): t-SNE of the pooled cells with the exact
// gradient.  Nothing of size N x N is stored: the conditional affinities and the joint probabilities live on the K-neighbour
// lists of jamie_self_knn (O(N K)), and the repulsive term is a streamed pass over all pairs of the 2-D layout with per-row
// accumulators.  DESIGN.md §19.
//
//   tsne_affinities_kernel   one wave per cell: the perplexity solve of sklearn's `_binary_search_perplexity` in fp64
//   tsne_mutual_kernel       one thread per (cell, slot): is the cell listed by its neighbour, and the joint value of the pair
//   tsne_fill_kernel         the CSR rows of P: a row's own K entries, then the cells that list it without being listed
//   tsne_repulsion_kernel    R_i = sum_j w^2 (y_i - y_j) and z_i = sum_j w, w = 1 / (1 + |y_i - y_j|^2): the hot loop
//   tsne_merge_kernel        the segments' partial sums of a row added in segment order; z per block of 256 rows
//   tsne_sum_kernel          fp64 totals in a fixed order (Z; the KL and gradient-norm history)
//   tsne_attract_kernel      one wave per row of P: A_i, the gradient, and on logging iterations the row's KL term
//   tsne_update_kernel       sklearn's `_gradient_descent` update, elementwise in fp32
//
// Deterministic: no floating-point atomics; every sum has one owner and a fixed order.
#include "lane_tree.h"
#include "mutual.h"

namespace {

constexpr int TS_KMAX = 128;      // neighbours per cell (jamie_self_knn's limit): two per lane of a wave
constexpr int SEG_TILE = 128;     // seg_rows is a multiple of it
constexpr int RPT = 4;            // rows of the layout a thread owns in registers
constexpr int ROWS = 256 * RPT;   // rows per workgroup
constexpr int CT = 512;           // columns (walked side) staged in LDS at a time: one float4 = two points per thread
constexpr int RUN = 32;           // columns per fp32 partial sum; the partial then goes into the fp64 accumulator
constexpr long long TARGET_BLOCKS = 1024;     // 4 workgroups of 256 threads (128 VGPRs) on each of 256 compute units: one round

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ---- step 2: conditional affinities ----
// lane l holds neighbours l and l + 64.  e_j = d_j^2 - d_1^2 (d_1 the nearest distance: slot 0), so the nearest neighbour has
// P = 1 at every beta and s >= 1: no cell can fail.
__device__ __forceinline__ double tsne_entropy(double beta, double e0, double e1, bool have0, bool have1, double& P0, double& P1,
                                               double& s) {
    P0 = have0 ? exp(-beta * e0) : 0.0;
    P1 = have1 ? exp(-beta * e1) : 0.0;
    s = wave_sum(P0 + P1);
    const double ep = wave_sum(e0 * P0 + e1 * P1);
    return log(s) + beta * ep / s;
}

__global__ __launch_bounds__(256) void tsne_affinities_kernel(const float* __restrict__ dist, long long N, int K, double log_u,
                                                              float* __restrict__ C, double* __restrict__ beta_out,
                                                              int32_t* __restrict__ tries_out) {
    const int lane = threadIdx.x & 63;
    const long long cell = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (cell >= N) return;                                 // (the whole wave)
    const bool have0 = lane < K, have1 = lane + 64 < K;
    const double d1 = (double)dist[cell * K];
    const double D0 = have0 ? (double)dist[cell * K + lane] : 0.0, D1 = have1 ? (double)dist[cell * K + lane + 64] : 0.0;
    const double e0 = have0 ? D0 * D0 - d1 * d1 : 0.0, e1 = have1 ? D1 * D1 - d1 * d1 : 0.0;
    const double inf = __builtin_inf();
    double beta = 1.0, bmin = -inf, bmax = inf, P0, P1, s;
    double diff = tsne_entropy(beta, e0, e1, have0, have1, P0, P1, s) - log_u;
    int tries = 0;
    while (fabs(diff) > 1e-5 && tries < 100) {             // (diff is the same bits in every lane: the wave branches as one)
        if (diff > 0.0) {
            bmin = beta;
            beta = bmax == inf ? beta * 2.0 : (beta + bmax) / 2.0;
        } else {
            bmax = beta;
            beta = bmin == -inf ? beta / 2.0 : (beta + bmin) / 2.0;
        }
        diff = tsne_entropy(beta, e0, e1, have0, have1, P0, P1, s) - log_u;
        ++tries;
    }
    if (have0) C[cell * K + lane] = (float)(P0 / s);
    if (have1) C[cell * K + lane + 64] = (float)(P1 / s);
    if (lane == 0) {
        beta_out[cell] = beta;
        tries_out[cell] = tries;
    }
}

// ---- step 3: joint probabilities ----
// (the two directions are added as doubles: a + b and b + a are the same bits, so P is symmetric to the bit)
__global__ __launch_bounds__(256) void tsne_mutual_kernel(const int32_t* __restrict__ idx, const float* __restrict__ C, long long N,
                                                          int K, float* __restrict__ val, int32_t* __restrict__ mutual) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= N * K) return;
    const long long i = e / K;
    const long long j = idx[e];
    double other;
    const int m = mutual_search(idx, C, N, K, i, j, other);
    val[e] = (float)(((double)C[e] + other) / (2.0 * (double)N));
    mutual[e] = m;
}

// thread t < N K: the own entry (i, slot) of row i; thread N K + r: the r-th one-directional pair in (target, then source) order,
// the entry of the TARGET's row behind its own K
__global__ __launch_bounds__(256) void tsne_fill_kernel(const int32_t* __restrict__ idx, const float* __restrict__ val, long long N,
                                                        int K, const long long* __restrict__ rowptr,
                                                        const long long* __restrict__ rev_pos, const int32_t* __restrict__ rev_tgt,
                                                        const long long* __restrict__ rev_start, long long n_rev, long long nnz,
                                                        int32_t* __restrict__ col, float* __restrict__ pval) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long NK = N * K;
    if (t < NK) {
        const long long o = rowptr[t / K] + t % K;
        if (o >= 0 && o < nnz) {
            col[o] = idx[t];
            pval[o] = val[t];
        }
    } else if (t - NK < n_rev) {
        const long long r = t - NK, j = rev_tgt[r], e = rev_pos[r];
        if (j < 0 || j >= N || e < 0 || e >= NK) return;
        const long long o = rowptr[j] + K + (r - rev_start[j]);
        if (o >= 0 && o < nnz) {
            col[o] = (int32_t)(e / K);
            pval[o] = val[e];
        }
    }
}

// ---- step 4: the repulsive term ----
// w = 1 / d, d = 1 + dx^2 + dy^2 >= 1: v_rcp_f32 and one Newton step (v_rcp_f32 alone is good to 1 ulp, but its error need not
// average out over the pairs of a row; after the step what is left is the rounding of the last fma)
__device__ __forceinline__ float tsne_weight(float dx, float dy, float& d) {
    d = __builtin_fmaf(dx, dx, __builtin_fmaf(dy, dy, 1.f));
    const float r = __builtin_amdgcn_rcpf(d);
    return __builtin_fmaf(__builtin_fmaf(-d, r, 1.f), r, r);
}

template <bool DIAG>
__device__ __forceinline__ void tsne_pair(const float2 c, int j, const float (&xi)[RPT], const float (&yi)[RPT], const int (&di)[RPT],
                                          float (&pz)[RPT], float (&px)[RPT], float (&py)[RPT]) {
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
        const float dx = xi[r] - c.x, dy = yi[r] - c.y;
        float d;
        float w = tsne_weight(dx, dy, d);
        if constexpr (DIAG) w = j == di[r] ? 0.f : w;      // the row itself, refused by index
        pz[r] += w;
        const float w2 = w * w;
        px[r] = __builtin_fmaf(w2, dx, px[r]);
        py[r] = __builtin_fmaf(w2, dy, py[r]);
    }
}

// nj staged columns against the thread's rows: fp32 partial sums over runs of RUN columns, each run added into the fp64 sums
template <bool DIAG>
__device__ __forceinline__ void tsne_chunk(const float2* __restrict__ Ys, int nj, const float (&xi)[RPT], const float (&yi)[RPT],
                                           const int (&di)[RPT], double (&az)[RPT], double (&ax)[RPT], double (&ay)[RPT]) {
    for (int j0 = 0; j0 < nj; j0 += RUN) {
        float pz[RPT], px[RPT], py[RPT];
#pragma unroll
        for (int r = 0; r < RPT; ++r) pz[r] = px[r] = py[r] = 0.f;
        if (nj - j0 >= RUN) {
#pragma unroll 8
            for (int k = 0; k < RUN; ++k) tsne_pair<DIAG>(Ys[j0 + k], j0 + k, xi, yi, di, pz, px, py);
        } else {
            for (int k = 0; k < nj - j0; ++k) tsne_pair<DIAG>(Ys[j0 + k], j0 + k, xi, yi, di, pz, px, py);
        }
#pragma unroll
        for (int r = 0; r < RPT; ++r) {
            az[r] += (double)pz[r];
            ax[r] += (double)px[r];
            ay[r] += (double)py[r];
        }
    }
}

// columns [c, c + 2) of Y below `lim` as one float4 (zeros where the column does not exist); c is even and Y is 16-byte aligned
__device__ __forceinline__ float4 tsne_load_pair(const float* __restrict__ Y, long long c, long long lim) {
    if (c + 1 < lim) return *reinterpret_cast<const float4*>(Y + 2 * c);
    if (c < lim) {
        const float2 v = *reinterpret_cast<const float2*>(Y + 2 * c);
        return make_float4(v.x, v.y, 0.f, 0.f);
    }
    return make_float4(0.f, 0.f, 0.f, 0.f);
}

// One workgroup: rows [blockIdx.x ROWS, + ROWS) against segment blockIdx.y of the columns.  Thread t owns rows row0 + r 256 + t.
// part is [S][3][N] fp64: z, R_x, R_y of a row over the segment.
__global__ __launch_bounds__(256, 4) void tsne_repulsion_kernel(const float* __restrict__ Y, long long N, long long seg_len,
                                                                double* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float2 Ys[CT];
    const long long row0 = (long long)blockIdx.x * ROWS;
    const long long c0 = (long long)blockIdx.y * seg_len;
    const long long c1 = c0 + seg_len < N ? c0 + seg_len : N;
    float xi[RPT], yi[RPT];
    double az[RPT], ax[RPT], ay[RPT];
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
        const long long gi = row0 + r * 256 + threadIdx.x;
        const float2 v = gi < N ? *reinterpret_cast<const float2*>(Y + 2 * gi) : make_float2(0.f, 0.f);
        xi[r] = v.x;
        yi[r] = v.y;
        az[r] = ax[r] = ay[r] = 0.0;
    }
    float4 next = tsne_load_pair(Y, c0 + 2 * threadIdx.x, c1);
    for (long long j0 = c0; j0 < c1; j0 += CT) {
        __syncthreads();                                   // the last chunk's reads are done
        *reinterpret_cast<float4*>(&Ys[2 * threadIdx.x]) = next;
        __syncthreads();
        if (j0 + CT < c1) next = tsne_load_pair(Y, j0 + CT + 2 * threadIdx.x, c1);      // (in flight under the arithmetic)
        const int nj = (int)(c1 - j0 < CT ? c1 - j0 : CT);
        if (j0 < row0 + ROWS && j0 + nj > row0) {          // the chunk holds rows of this workgroup (the same answer in every thread)
            int di[RPT];
#pragma unroll
            for (int r = 0; r < RPT; ++r) {
                const long long d = row0 + r * 256 + threadIdx.x - j0;
                di[r] = d >= 0 && d < nj ? (int)d : -1;
            }
            tsne_chunk<true>(Ys, nj, xi, yi, di, az, ax, ay);
        } else {
            const int di[RPT] = {};
            tsne_chunk<false>(Ys, nj, xi, yi, di, az, ax, ay);
        }
    }
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
        const long long gi = row0 + r * 256 + threadIdx.x;
        if (gi < N) {
            double* p = part + (long long)blockIdx.y * 3 * N + gi;
            p[0] = az[r];
            p[N] = ax[r];
            p[2 * N] = ay[r];
        }
    }
}

// the workgroup's 256 values added by the tree v[t] += v[t + s], s = 128, 64, ..., 1; the total is valid in thread 0
__device__ __forceinline__ double block_tree_f64(double v, double* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(256) void tsne_merge_kernel(const double* __restrict__ part, long long N, int S, double* __restrict__ R,
                                                         double* __restrict__ z, double* __restrict__ zpart) {
    __shared__ double red[256];
    const long long gi = (long long)blockIdx.x * 256 + threadIdx.x;
    double sz = 0.0, sx = 0.0, sy = 0.0;
    if (gi < N) {
        for (int s = 0; s < S; ++s) {
            const double* p = part + (long long)s * 3 * N + gi;
            sz += p[0];
            sx += p[N];
            sy += p[2 * N];
        }
        R[2 * gi] = sx;
        R[2 * gi + 1] = sy;
        z[gi] = sz;
    }
    const double t = block_tree_f64(sz, red);
    if (threadIdx.x == 0) zpart[blockIdx.x] = t;
}

// *out = the sum of in[0 .. n), one workgroup: thread t adds elements t, t + 256, ... in ascending order, then the tree of
// block_tree_f64
__global__ __launch_bounds__(256) void tsne_sum_kernel(const double* __restrict__ in, long long n, double* __restrict__ out) {
    __shared__ double red[256];
    double s = 0.0;
    for (long long i = threadIdx.x; i < n; i += 256) s += in[i];
    const double t = block_tree_f64(s, red);
    if (threadIdx.x == 0) *out = t;
}

// ---- the attractive term, the gradient, the update ----
// One wave per row of P: lane l takes entries l, l + 64, ... of the row in fp32, adds them as doubles, and the lanes are added by
// the xor tree.  logbuf [2][N] (may be NULL): the row's KL term and the square of its gradient.
__global__ __launch_bounds__(256) void tsne_attract_kernel(const long long* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                           const float* __restrict__ val, long long nnz, const float* __restrict__ Y,
                                                           long long N, const double* __restrict__ R, const double* __restrict__ Zp,
                                                           double alpha, float* __restrict__ grad, double* __restrict__ A_out,
                                                           double* __restrict__ logbuf) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;                                  // (the whole wave)
    const float xi = Y[2 * row], yi = Y[2 * row + 1];
    long long e0 = rowptr[row], e1 = rowptr[row + 1];
    e0 = e0 < 0 ? 0 : e0;
    e1 = e1 > nnz ? nnz : e1;
    const double Z = *Zp;
    double ax = 0.0, ay = 0.0, kl = 0.0;
    for (long long e = e0 + lane; e < e1; e += 64) {
        const long long j = col[e];
        if (j < 0 || j >= N) continue;
        const float p = val[e];
        const float dx = xi - Y[2 * j], dy = yi - Y[2 * j + 1];
        float d;
        const float pw = p * tsne_weight(dx, dy, d);
        ax += (double)(pw * dx);
        ay += (double)(pw * dy);
        if (logbuf && p > 0.f) kl += (double)p * log((double)p * (double)d * Z);
    }
    ax = wave_sum(ax);
    ay = wave_sum(ay);
    if (logbuf) kl = wave_sum(kl);
    if (lane == 0) {
        const float gx = (float)(4.0 * (alpha * ax - R[2 * row] / Z)), gy = (float)(4.0 * (alpha * ay - R[2 * row + 1] / Z));
        grad[2 * row] = gx;
        grad[2 * row + 1] = gy;
        if (A_out) {
            A_out[2 * row] = ax;
            A_out[2 * row + 1] = ay;
        }
        if (logbuf) {
            logbuf[row] = kl;
            logbuf[N + row] = (double)gx * (double)gx + (double)gy * (double)gy;
        }
    }
}

__global__ __launch_bounds__(256) void tsne_update_kernel(const float* __restrict__ grad, long long n, float momentum, float lr,
                                                          float* __restrict__ Y, float* __restrict__ u, float* __restrict__ gain) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const float g = grad[t];
    float uu = u[t], gn = gain[t];
    gn = uu * g < 0.f ? gn + 0.2f : gn * 0.8f;
    gn = gn < 0.01f ? 0.01f : gn;
    uu = momentum * uu - lr * (gn * g);
    gain[t] = gn;
    u[t] = uu;
    Y[t] += uu;
}

// rows of Y per segment of the walked side: the caller's, or whole 128-column tiles spread evenly over the number of segments
// that brings the launch closest to TARGET_BLOCKS workgroups from below
inline long long tsne_seg_len(long long N, long long seg_rows) {
    if (seg_rows > 0) return seg_rows;
    const long long rb = (N + ROWS - 1) / ROWS, tiles = (N + SEG_TILE - 1) / SEG_TILE;
    long long S = TARGET_BLOCKS / rb;
    S = S < 1 ? 1 : (S > tiles ? tiles : S);
    return (tiles + S - 1) / S * SEG_TILE;
}

inline long long round16(long long b) { return (b + 15) / 16 * 16; }

}  // namespace

extern "C" int jamie_tsne_affinities(const float* dist, long long N, int K, double perplexity, float* C, double* beta, int32_t* tries,
                                     void* stream) {
    JAMIE_ARG(dist && C && beta && tries, "null pointer");
    JAMIE_ARG(N >= 1 && K >= 2 && K <= TS_KMAX, "N >= 1, 2 <= K <= 128");
    JAMIE_ARG(perplexity > 1.0 && perplexity < (double)K, "1 < perplexity < K");
    JAMIE_ARG((N + 3) / 4 <= 2147483647ll, "N too large for one launch");
    hipLaunchKernelGGL(tsne_affinities_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, (hipStream_t)stream, dist, N, K,
                       log(perplexity), C, beta, tries);
    return jamie_launch_status("jamie_tsne_affinities");
}

extern "C" int jamie_tsne_mutual(const int32_t* idx, const float* C, long long N, int K, float* val, int32_t* mutual, void* stream) {
    JAMIE_ARG(idx && C && val && mutual, "null pointer");
    JAMIE_ARG(N >= 1 && N < 2147483647ll && K >= 1 && K <= TS_KMAX, "1 <= N < 2^31, 1 <= K <= 128");
    const long long blocks = (N * K + 255) / 256;
    JAMIE_ARG(blocks <= 2147483647ll, "N K too large for one launch");
    hipLaunchKernelGGL(tsne_mutual_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, idx, C, N, K, val, mutual);
    return jamie_launch_status("jamie_tsne_mutual");
}

extern "C" int jamie_tsne_fill(const int32_t* idx, const float* val, long long N, int K, const long long* rowptr,
                               const long long* rev_pos, const int32_t* rev_tgt, const long long* rev_start, long long n_rev,
                               int32_t* col, float* pval, void* stream) {
    JAMIE_ARG(idx && val && rowptr && rev_start && col && pval, "null pointer");
    JAMIE_ARG(N >= 1 && N < 2147483647ll && K >= 1 && K <= TS_KMAX, "1 <= N < 2^31, 1 <= K <= 128");
    JAMIE_ARG(n_rev >= 0 && n_rev <= N * K && (n_rev == 0 || (rev_pos && rev_tgt)), "0 <= n_rev <= N K, with its two arrays");
    const long long blocks = (N * K + n_rev + 255) / 256;
    JAMIE_ARG(blocks <= 2147483647ll, "N K too large for one launch");
    hipLaunchKernelGGL(tsne_fill_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, idx, val, N, K, rowptr, rev_pos,
                       rev_tgt, rev_start, n_rev, N * K + n_rev, col, pval);
    return jamie_launch_status("jamie_tsne_fill");
}

extern "C" long long jamie_tsne_repulsion_workspace(long long N, long long seg_rows) {
    if (N < 2 || N >= 2147483647ll || seg_rows < 0 || seg_rows % SEG_TILE != 0) return 0;
    const long long seg_len = tsne_seg_len(N, seg_rows);
    const long long S = (N + seg_len - 1) / seg_len;
    return round16(S * 3 * N * 8) + round16((N + 255) / 256 * 8);
}

extern "C" int jamie_tsne_repulsion(const float* Y, long long N, double* R, double* z, double* Z, long long seg_rows, void* ws,
                                    long long ws_bytes, void* stream) {
    JAMIE_ARG(Y && R && z && Z && ws, "null pointer");
    JAMIE_ARG(N >= 2 && N < 2147483647ll, "2 <= N < 2^31");
    JAMIE_ARG(seg_rows >= 0 && seg_rows % SEG_TILE == 0, "seg_rows is 0 or a positive multiple of 128");
    JAMIE_ARG(aligned16(Y) && aligned16(ws), "Y and ws must be 16-byte aligned");
    const long long seg_len = tsne_seg_len(N, seg_rows);
    const long long S = (N + seg_len - 1) / seg_len;
    JAMIE_ARG(S <= 65535, "at most 65535 segments");
    JAMIE_ARG(ws_bytes >= jamie_tsne_repulsion_workspace(N, seg_rows), "workspace smaller than jamie_tsne_repulsion_workspace(N, seg_rows)");
    hipStream_t st = (hipStream_t)stream;
    double* part = (double*)ws;
    double* zpart = (double*)((char*)ws + round16(S * 3 * N * 8));
    const long long nb = (N + 255) / 256;
    hipLaunchKernelGGL(tsne_repulsion_kernel, dim3((unsigned)((N + ROWS - 1) / ROWS), (unsigned)S), dim3(256), 0, st, Y, N, seg_len, part);
    hipLaunchKernelGGL(tsne_merge_kernel, dim3((unsigned)nb), dim3(256), 0, st, (const double*)part, N, (int)S, R, z, zpart);
    hipLaunchKernelGGL(tsne_sum_kernel, dim3(1), dim3(256), 0, st, (const double*)zpart, nb, Z);
    return jamie_launch_status("jamie_tsne_repulsion");
}

extern "C" long long jamie_tsne_step_workspace(long long N) {
    if (N < 2 || N >= 2147483647ll) return 0;
    return round16(2 * N * 8) + round16(2 * N * 4);
}

extern "C" int jamie_tsne_step(const long long* rowptr, const int32_t* col, const float* val, long long nnz, float* Y, long long N,
                               const double* R, const double* Z, double alpha, double momentum, double lr, float* u, float* gain,
                               int update, float* grad, double* A, double* kl, double* gsq, void* ws, long long ws_bytes, void* stream) {
    JAMIE_ARG(rowptr && col && val && Y && R && Z && ws, "null pointer");
    JAMIE_ARG(N >= 2 && N < 2147483647ll && nnz >= 0, "2 <= N < 2^31, nnz >= 0");
    JAMIE_ARG(!update || (u && gain), "an update needs u and gain");
    JAMIE_ARG((kl == nullptr) == (gsq == nullptr), "kl and gsq are given together");
    JAMIE_ARG(alpha >= 1.0 && momentum >= 0.0 && lr > 0.0, "alpha >= 1, momentum >= 0, lr > 0");
    JAMIE_ARG(ws_bytes >= jamie_tsne_step_workspace(N), "workspace smaller than jamie_tsne_step_workspace(N)");
    JAMIE_ARG((N + 3) / 4 <= 2147483647ll, "N too large for one launch");
    hipStream_t st = (hipStream_t)stream;
    double* logbuf = (double*)ws;
    float* g = grad ? grad : (float*)((char*)ws + round16(2 * N * 8));
    hipLaunchKernelGGL(tsne_attract_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, rowptr, col, val, nnz, (const float*)Y, N, R,
                       Z, alpha, g, A, kl ? logbuf : (double*)nullptr);
    if (kl) {
        hipLaunchKernelGGL(tsne_sum_kernel, dim3(1), dim3(256), 0, st, (const double*)logbuf, N, kl);
        hipLaunchKernelGGL(tsne_sum_kernel, dim3(1), dim3(256), 0, st, (const double*)(logbuf + N), N, gsq);
    }
    if (update)
        hipLaunchKernelGGL(tsne_update_kernel, dim3((unsigned)((2 * N + 255) / 256)), dim3(256), 0, st, (const float*)g, 2 * N,
                           (float)momentum, (float)lr, Y, u, gain);
    return jamie_launch_status("jamie_tsne_step");
}

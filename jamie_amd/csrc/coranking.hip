// Layout quality on the device (include/jamie_hip.h "Layout quality on the device"; jamie_amd/coranking.py): the rank, in the
// space X, of every entry of a neighbour list -- rank[i, t] = #{ l != i : (q(i, l), l) < (q(i, j), j) }, j = idx[i, t] -- as one
// streaming pass over the pair space of X.  Nothing of size N x N is stored.  q, the pair tile and the order `key_less` are
// pair_tile.h's; the threshold q(i, j) of every entry is formed first, by the same chain, so both sides of every comparison carry
// the same rounding (what jamie_foscttm_counts does for q(i, i)).  Counts are integers: any order of adding them gives the same
// bits.
#include "pair_tile.h"

namespace {

// thr[i, t] = q(i, idx[i, t]) by the chain of pair_tile, NaN read as +inf; -1 for an entry that is not ranked (j == i, j outside
// [0, N)): below every q, so such an entry sorts in front of the row's thresholds and no pair is ever under it.  rank starts at 0
// (-1 where not ranked): the pass adds to it.
__global__ __launch_bounds__(256) void list_threshold_kernel(const float* __restrict__ X, long long N, int L,
                                                             const int32_t* __restrict__ idx, int K, float* __restrict__ thr,
                                                             int32_t* __restrict__ rank) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= N * K) return;
    const long long i = e / K;
    const long long j = idx[e];
    if (j < 0 || j >= N || j == i) {
        thr[e] = -1.f;
        rank[e] = -1;
        return;
    }
    const float* a = X + i * L;
    const float* b = X + j * L;
    float q = 0.f;
    for (int c = 0; c < L; ++c) q = q_step(q, a[c], b[c]);
    thr[e] = q == q ? q : __builtin_inff();
    rank[e] = 0;
}

// first position of the row's sorted thresholds whose key is above (ABOVE) / not below (!ABOVE) the key (q, j)
template <bool ABOVE>
__device__ __forceinline__ int threshold_search(const float* __restrict__ tq, const int* __restrict__ tj, int K, float q, int j) {
    int lo = 0, hi = K;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const float mq = tq[mid];
        const int mj = tj[mid];
        const bool left = ABOVE ? key_less(q, j, mq, mj) : !key_less(mq, mj, q, j);
        hi = left ? mid : hi;
        lo = left ? lo : mid + 1;
    }
    return lo;
}

// One workgroup: MI * 64 rows against segment blockIdx.y of the rows of X, 128 at a time.  The rows' K thresholds sit in LDS,
// sorted by key; a thread tests the minimum of each of its rows' 8 q against the row's largest threshold (a NaN q drops out of
// v_min_f32, and is below nothing unless that threshold is +inf, which every q passes), and a q that passes is placed among the
// row's thresholds by a binary search: one LDS integer add into hist[row][b], b the number of thresholds not above the pair's key.
// The rank of the threshold at sorted position s is hist[row][0] + .. + hist[row][s].  Two shapes, as the neighbour search: 128
// rows with up to 16 thresholds, 64 rows with up to 64.
template <int MI, int KP>
__global__ __launch_bounds__(256, 2) void list_ranks_kernel(const float* __restrict__ X, long long N, int L, int vec,
                                                            const int32_t* __restrict__ idx, const float* __restrict__ thr, int K,
                                                            long long tile_i0, long long seg_len, int32_t* __restrict__ rank) {
    constexpr int QT = MI * 64;
    constexpr int LDK = KP + 1;                            // (+1: the rows' lists start on different banks)
    __shared__ __attribute__((aligned(16))) float smem[KC * (QT + 4) + KC * LDJ];
    __shared__ float tq[QT * LDK];
    __shared__ int tj[QT * LDK];
    __shared__ int hist[QT * LDK];
    float* Xs = smem;
    float* Ys = smem + KC * (QT + 4);
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const long long i0 = (tile_i0 + blockIdx.x) * QT;
    const long long r0 = (long long)blockIdx.y * seg_len;
    const long long r1 = r0 + seg_len < N ? r0 + seg_len : N;

    // the thresholds, sorted by (q, index), equal keys in the caller's order: K^2 counting on the keys as they came, which wait
    // in the space of the staged operands (q) and of the histogram (index)
    float* rq = smem;
    int* rj = hist;
#pragma unroll 1
    for (int s = threadIdx.x; s < QT * KP; s += 256) {
        const int row = s / KP, t = s % KP;
        const long long gi = i0 + row;
        const bool have = t < K && gi < N;
        rq[s] = have ? thr[gi * K + t] : -1.f;
        rj[s] = have ? idx[gi * K + t] : 0;
    }
    __syncthreads();
#pragma unroll 1
    for (int s = threadIdx.x; s < QT * KP; s += 256) {
        const int row = s / KP, t = s % KP;
        if (t >= K) continue;
        const float q = rq[s];
        const int j = rj[s];
        int p = 0;
        for (int o = 0; o < K; ++o) {
            const float oq = rq[row * KP + o];
            const int oj = rj[row * KP + o];
            p += key_less(oq, oj, q, j) || (oq == q && oj == j && o < t) ? 1 : 0;
        }
        tq[row * LDK + p] = q;
        tj[row * LDK + p] = j;
    }
    __syncthreads();
    for (int s = threadIdx.x; s < QT * LDK; s += 256) hist[s] = 0;
    // (the barriers inside pair_tile stand between this and the first add, and between the reads above and the staging)
    float tmax[MI * 4];
#pragma unroll
    for (int r = 0; r < MI * 4; ++r) tmax[r] = tq[((r >> 2) * 64 + ty * 4 + (r & 3)) * LDK + K - 1];

    for (long long j0 = r0; j0 < r1; j0 += TJ) {
        float acc[MI * 4][8];
        pair_tile<MI>(X, N, i0, X, r1, j0, L, vec != 0, Xs, Ys, acc);
#pragma unroll
        for (int r = 0; r < MI * 4; ++r) {
            const float lo = __builtin_fminf(
                __builtin_fminf(__builtin_fminf(acc[r][0], acc[r][1]), __builtin_fminf(acc[r][2], acc[r][3])),
                __builtin_fminf(__builtin_fminf(acc[r][4], acc[r][5]), __builtin_fminf(acc[r][6], acc[r][7])));
            if (lo > tmax[r]) continue;                    // (a NaN minimum: all 8 are NaN; the search below reads them as +inf)
            unsigned todo = 0;
#pragma unroll
            for (int s = 0; s < 8; ++s) todo |= acc[r][s] > tmax[r] ? 0u : 1u << s;
            const int row = (r >> 2) * 64 + ty * 4 + (r & 3);
            const long long gi = i0 + row;
            for (; todo; todo &= todo - 1) {
                const int s = __ffs((int)todo) - 1;
                float q = acc[r][0];
#pragma unroll
                for (int o = 1; o < 8; ++o) q = s == o ? acc[r][o] : q;
                const long long gj = j0 + (s >> 2) * 64 + tx * 4 + (s & 3);
                if (gj >= r1 || gj == gi) continue;        // rows that do not exist; the cell itself, by index
                q = q == q ? q : __builtin_inff();
                const int b = threshold_search<true>(&tq[row * LDK], &tj[row * LDK], K, q, (int)gj);
                if (b < K) atomicAdd(&hist[row * LDK + b], 1);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < QT) {
        int sum = 0;
        for (int s = 0; s < K; ++s) {
            sum += hist[threadIdx.x * LDK + s];
            hist[threadIdx.x * LDK + s] = sum;
        }
    }
    __syncthreads();
    // back to the caller's order: an entry finds the first sorted position of its own key (equal keys share a rank: no pair lies
    // between them)
#pragma unroll 1
    for (int s = threadIdx.x; s < QT * KP; s += 256) {
        const int row = s / KP, t = s % KP;
        const long long gi = i0 + row;
        if (t >= K || gi >= N) continue;
        const float q = thr[gi * K + t];
        if (!(q >= 0.f)) continue;                         // not ranked: stays -1
        const int p = threshold_search<false>(&tq[row * LDK], &tj[row * LDK], K, q, idx[gi * K + t]);
        const int n = hist[row * LDK + p];
        if (n) atomicAdd(&rank[gi * K + t], n);
    }
}

// One thread per cell: for every k <= K the cell's penalty sum_{p < k} max(0, rank[i, p] + 1 - k) and its count of entries p < k
// with rank < k, summed over the cells of a workgroup by waves and LDS, then one global integer add per k and workgroup.
__global__ __launch_bounds__(256) void coranking_sums_kernel(const int32_t* __restrict__ rank, long long N, int K,
                                                             unsigned long long* __restrict__ penalty,
                                                             unsigned long long* __restrict__ overlap,
                                                             long long* __restrict__ cell_penalty) {
    __shared__ unsigned long long spen[KMAX], sov[KMAX];
    if (threadIdx.x < KMAX) {
        spen[threadIdx.x] = 0;
        sov[threadIdx.x] = 0;
    }
    __syncthreads();
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int32_t* row = rank + i * K;
    for (int k = 1; k <= K; ++k) {
        long long pen = 0, ov = 0;
        if (i < N)
            for (int p = 0; p < k; ++p) {
                const int r = row[p];
                pen += r >= k ? r + 1 - k : 0;
                ov += r >= 0 && r < k ? 1 : 0;
            }
        if (k == K && i < N) cell_penalty[i] = pen;
        for (int d = 32; d; d >>= 1) {
            pen += __shfl_down(pen, d);
            ov += __shfl_down(ov, d);
        }
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(&spen[k - 1], (unsigned long long)pen);
            atomicAdd(&sov[k - 1], (unsigned long long)ov);
        }
    }
    __syncthreads();
    if (threadIdx.x < K) {
        atomicAdd(&penalty[threadIdx.x], spen[threadIdx.x]);
        atomicAdd(&overlap[threadIdx.x], sov[threadIdx.x]);
    }
}

// rows of X per segment: the caller's, or the library's count of equally long segments (the rule of jamie_self_knn)
inline long long ranks_seg_len(long long N, int K, long long seg_rows) {
    if (seg_rows > 0) return seg_rows;
    const int S = knn_segments(N, N, K);
    return ((N + S - 1) / S + TJ - 1) / TJ * TJ;
}

}  // namespace

extern "C" long long jamie_list_ranks_workspace(long long N, int K, long long seg_rows) {
    if (N < 2 || N >= 2147483647ll || K < 1 || K > KMAX || seg_rows < 0 || seg_rows % TJ != 0) return 0;
    return N * K * 4;
}

extern "C" int jamie_list_ranks(const float* X, long long N, int L, const int32_t* idx, int K, int32_t* rank, long long seg_rows,
                                void* ws, long long ws_bytes, void* stream) {
    JAMIE_ARG(N >= 2 && N < 2147483647ll && L >= 1, "2 <= N < 2^31, L >= 1");
    JAMIE_ARG(K >= 1 && K <= KMAX, "1 <= K <= 64");
    JAMIE_ARG(seg_rows >= 0 && seg_rows % TJ == 0, "seg_rows is 0 or a positive multiple of 128");
    JAMIE_ARG(X && idx && rank && ws, "null pointer");
    const long long seg_len = ranks_seg_len(N, K, seg_rows);
    const long long S = (N + seg_len - 1) / seg_len;
    JAMIE_ARG(S <= 65535, "at most 65535 segments");
    JAMIE_ARG(ws_bytes >= jamie_list_ranks_workspace(N, K, seg_rows), "workspace smaller than jamie_list_ranks_workspace(N, K, seg_rows)");
    hipStream_t st = (hipStream_t)stream;
    float* thr = (float*)ws;
    hipLaunchKernelGGL(list_threshold_kernel, dim3((unsigned)((N * K + 255) / 256)), dim3(256), 0, st, X, N, L, idx, K, thr, rank);
    const int QT = knn_query_tile(K);
    const int vec = (L % 4 == 0) && aligned16(X);
    const long long nt = (N + QT - 1) / QT;
    const long long step = tiles_per_launch(N, L, QT);
    for (long long t0 = 0; t0 < nt; t0 += step) {
        const long long n = nt - t0 < step ? nt - t0 : step;
        if (QT == 128)
            hipLaunchKernelGGL((list_ranks_kernel<2, K_SMALL>), dim3((unsigned)n, (unsigned)S), dim3(256), 0, st, X, N, L, vec, idx,
                               (const float*)thr, K, t0, seg_len, rank);
        else
            hipLaunchKernelGGL((list_ranks_kernel<1, KMAX>), dim3((unsigned)n, (unsigned)S), dim3(256), 0, st, X, N, L, vec, idx,
                               (const float*)thr, K, t0, seg_len, rank);
    }
    return jamie_launch_status("jamie_list_ranks");
}

extern "C" int jamie_coranking_sums(const int32_t* rank, long long N, int K, long long* penalty, long long* overlap,
                                    long long* cell_penalty, void* stream) {
    JAMIE_ARG(rank && penalty && overlap && cell_penalty, "null pointer");
    JAMIE_ARG(N >= 1 && K >= 1 && K <= KMAX, "N >= 1, 1 <= K <= 64");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(penalty, 0, K * 8, st) != hipSuccess || hipMemsetAsync(overlap, 0, K * 8, st) != hipSuccess)
        return jamie_launch_status("jamie_coranking_sums");
    hipLaunchKernelGGL(coranking_sums_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, rank, N, K,
                       (unsigned long long*)penalty, (unsigned long long*)overlap, cell_penalty);
    return jamie_launch_status("jamie_coranking_sums");
}

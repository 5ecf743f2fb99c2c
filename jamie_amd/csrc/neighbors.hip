// Neighbourhoods on the device (include/jamie_hip.h "Neighbourhoods on the device"; jamie_amd/neighbors.py): the K nearest OTHER
// rows of one [N, L] fp32 matrix, K <= 128, and the local inverse Simpson index (LISI, Korsunsky et al. 2019) on such lists.
// Nothing of size N x N is stored.
//
// The search is the workgroup of the cross search (pair_tile.h `knn_partial_kernel`) with the query's own row refused by index.
// A list holds at most 64 entries, one per lane of a wave, so K > 64 is two passes: the first leaves the 64 nearest, the second
// walks the rows again, admits only what lies above the query's 64th key (q, index) and selects the K - 64 smallest of that.
// (q, index) is a total order and both passes form q by the same chain, so a candidate falls on the same side of the floor in
// both and the concatenation is exactly the K smallest: no tie across the seam is lost or taken twice.
#include "lane_tree.h"
#include "pair_tile.h"

namespace {

constexpr int SELF_KMAX = 2 * KMAX;

// a wave per query: the segments' lists (of the candidates above `floor`, if given) offered in segment order; idx and sqrt(q) go
// to columns [col0, col0 + K) of the [Nq, ldo] outputs, the last entry's key to floor_out (the floor of the next pass)
__global__ __launch_bounds__(256) void self_knn_merge_kernel(const float* __restrict__ part_q, const int* __restrict__ part_i,
                                                             long long Nq, int K, int S, const float* __restrict__ floor_q,
                                                             const int* __restrict__ floor_i, int32_t* __restrict__ idx,
                                                             float* __restrict__ dist, int ldo, int col0,
                                                             float* __restrict__ floor_q_out, int* __restrict__ floor_i_out) {
    const int lane = threadIdx.x & 63;
    const long long gq = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gq >= Nq) return;
    const float fq = floor_q ? floor_q[gq] : 0.f;
    const int fi = floor_q ? floor_i[gq] : 0;
    float mq = __builtin_inff();
    int mi = 0x7fffffff;
    for (int s = 0; s < S; ++s) {
        const long long o = ((long long)s * Nq + gq) * K + lane;
        const bool have = lane < K;
        const float cq = have ? part_q[o] : 0.f;
        const int ci = have ? part_i[o] : 0;
        const bool valid = have && ci != 0x7fffffff && (!floor_q || key_less(fq, fi, cq, ci));
        wave_topk_offer(cq, ci, valid, K, mq, mi);
    }
    if (lane < K) {
        idx[gq * ldo + col0 + lane] = mi;
        dist[gq * ldo + col0 + lane] = sqrtf(mq);
    }
    if (floor_q_out && lane == K - 1) {
        floor_q_out[gq] = mq;
        floor_i_out[gq] = mi;
    }
}

// ---- LISI: one wave per cell, lane l holds neighbours l and l + 64; every sum over the neighbours is a fixed lane tree in fp64 ----
// (the fp64 lane tree `wave_sum` and `lane_value` are in lane_tree.h, shared with csrc/tsne.hip)
// H and the normalised weights of `compute_simpson_index` (Hbeta): P_j = exp(-D_j beta), s = sum P; s == 0: H = 0, P = 0; else
// H = log(s) + beta sum(D_j P_j) / s, P_j /= s
__device__ __forceinline__ double entropy_at(double beta, double D0, double D1, bool have0, bool have1, double& P0, double& P1) {
    P0 = have0 ? exp(-D0 * beta) : 0.0;
    P1 = have1 ? exp(-D1 * beta) : 0.0;
    const double s = wave_sum(P0 + P1);
    if (s == 0.0) {
        P0 = 0.0;
        P1 = 0.0;
        return 0.0;
    }
    const double dp = wave_sum(D0 * P0 + D1 * P1);
    P0 /= s;
    P1 /= s;
    return log(s) + beta * dp / s;
}

__global__ __launch_bounds__(256) void lisi_kernel(const int32_t* __restrict__ idx, const float* __restrict__ dist, long long N, int K,
                                                   const int32_t* __restrict__ codes, int n_sets, double log_u,
                                                   double* __restrict__ lisi, int32_t* __restrict__ tries_out) {
    const int lane = threadIdx.x & 63;
    const long long cell = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (cell >= N) return;                                 // (the whole wave)
    const bool have0 = lane < K, have1 = lane + 64 < K;
    const long long j0 = have0 ? idx[cell * K + lane] : -1, j1 = have1 ? idx[cell * K + lane + 64] : -1;
    const double D0 = have0 ? (double)dist[cell * K + lane] : 0.0, D1 = have1 ? (double)dist[cell * K + lane + 64] : 0.0;
    const double inf = __builtin_inf();
    double beta = 1.0, bmin = -inf, bmax = inf, P0, P1;
    double H = entropy_at(beta, D0, D1, have0, have1, P0, P1);
    double diff = H - log_u;
    int tries = 0;
    while (fabs(diff) > 1e-5 && tries < 50) {              // (H is the same bits in every lane: the wave branches as one)
        if (diff > 0.0) {
            bmin = beta;
            beta = bmax == inf ? beta * 2.0 : (beta + bmax) / 2.0;
        } else {
            bmax = beta;
            beta = bmin == -inf ? beta / 2.0 : (beta + bmin) / 2.0;
        }
        H = entropy_at(beta, D0, D1, have0, have1, P0, P1);
        diff = H - log_u;
        ++tries;
    }
    if (tries_out && lane == 0) tries_out[cell] = tries;
    for (int set = 0; set < n_sets; ++set) {
        // Simpson = sum_e P_e * (sum over f with code_f == code_e of P_f): K^2 compares, no table of the categories
        const int32_t* cs = codes + (long long)set * N;
        const int c0 = j0 >= 0 && j0 < N ? cs[j0] : -1, c1 = j1 >= 0 && j1 < N ? cs[j1] : -1;
        double in0 = 0.0, in1 = 0.0;
        for (int f = 0; f < K; ++f) {
            const double pf = f < 64 ? lane_value(P0, f) : lane_value(P1, f - 64);
            const int cf = f < 64 ? lane_value(c0, f) : lane_value(c1, f - 64);
            in0 += cf == c0 ? pf : 0.0;
            in1 += cf == c1 ? pf : 0.0;
        }
        const double simpson = wave_sum((have0 ? P0 * in0 : 0.0) + (have1 ? P1 * in1 : 0.0));
        if (lane == 0) lisi[(long long)set * N + cell] = H == 0.0 ? __builtin_nan("") : 1.0 / simpson;
    }
}

// rows of X per segment: the caller's, or the library's count of equally long segments
inline long long self_seg_len(long long N, int K, long long seg_rows) {
    if (seg_rows > 0) return seg_rows;
    const int S = knn_segments(N, N, K < KMAX ? K : KMAX);
    return ((N + S - 1) / S + TJ - 1) / TJ * TJ;
}

template <bool FLOOR>
void launch_self_pass(const float* X, long long N, int L, int K, long long seg_len, int S, const float* floor_q, const int* floor_i,
                      float* part_q, int* part_i, hipStream_t st) {
    const int QT = knn_query_tile(K);
    const int vec = (L % 4 == 0) && aligned16(X);
    const long long nt = (N + QT - 1) / QT;
    const long long step = tiles_per_launch(N, L, QT);
    for (long long t0 = 0; t0 < nt; t0 += step) {
        const long long n = nt - t0 < step ? nt - t0 : step;
        if (QT == 128)
            hipLaunchKernelGGL((knn_partial_kernel<2, K_SMALL, true, FLOOR>), dim3((unsigned)n, (unsigned)S), dim3(256), 0, st, X, N, X,
                               N, L, vec, K, t0, seg_len, floor_q, floor_i, part_q, part_i);
        else
            hipLaunchKernelGGL((knn_partial_kernel<1, KMAX, true, FLOOR>), dim3((unsigned)n, (unsigned)S), dim3(256), 0, st, X, N, X, N,
                               L, vec, K, t0, seg_len, floor_q, floor_i, part_q, part_i);
    }
}

}  // namespace

extern "C" long long jamie_self_knn_workspace(long long N, int K, long long seg_rows) {
    if (N < 2 || K < 1 || K > SELF_KMAX || seg_rows < 0 || seg_rows % TJ != 0) return 0;
    const long long seg_len = self_seg_len(N, K, seg_rows);
    const long long S = (N + seg_len - 1) / seg_len;
    return S * N * (K < KMAX ? K : KMAX) * 8 + (K > KMAX ? N * 8 : 0);
}

extern "C" int jamie_self_knn(const float* X, long long N, int L, int K, int32_t* idx, float* dist, long long seg_rows, void* ws,
                              long long ws_bytes, void* stream) {
    JAMIE_ARG(N >= 2 && N < 2147483647ll && L >= 1, "2 <= N < 2^31, L >= 1");
    JAMIE_ARG(K >= 1 && K <= SELF_KMAX && K <= N - 1, "1 <= K <= min(N - 1, 128)");
    JAMIE_ARG(seg_rows >= 0 && seg_rows % TJ == 0, "seg_rows is 0 or a positive multiple of 128");
    JAMIE_ARG(X && idx && dist && ws, "null pointer");
    const long long seg_len = self_seg_len(N, K, seg_rows);
    const long long S = (N + seg_len - 1) / seg_len;
    JAMIE_ARG(S <= 65535, "at most 65535 segments");
    JAMIE_ARG(ws_bytes >= jamie_self_knn_workspace(N, K, seg_rows), "workspace smaller than jamie_self_knn_workspace(N, K, seg_rows)");
    hipStream_t st = (hipStream_t)stream;
    const int K1 = K < KMAX ? K : KMAX, K2 = K - K1;
    float* part_q = (float*)ws;
    int* part_i = (int*)ws + S * N * K1;
    float* floor_q = K2 ? (float*)ws + 2 * S * N * K1 : nullptr;
    int* floor_i = K2 ? (int*)floor_q + N : nullptr;
    const dim3 mgrid((unsigned)((N + 3) / 4));
    launch_self_pass<false>(X, N, L, K1, seg_len, (int)S, nullptr, nullptr, part_q, part_i, st);
    hipLaunchKernelGGL(self_knn_merge_kernel, mgrid, dim3(256), 0, st, part_q, part_i, N, K1, (int)S, (const float*)nullptr,
                       (const int*)nullptr, idx, dist, K, 0, floor_q, floor_i);
    if (K2) {
        // the lists of the second pass take the place of the first's: [S, N, K2] in front of the same two halves
        launch_self_pass<true>(X, N, L, K2, seg_len, (int)S, floor_q, floor_i, part_q, part_i, st);
        hipLaunchKernelGGL(self_knn_merge_kernel, mgrid, dim3(256), 0, st, part_q, part_i, N, K2, (int)S, (const float*)floor_q,
                           (const int*)floor_i, idx, dist, K, K1, (float*)nullptr, (int*)nullptr);
    }
    return jamie_launch_status("jamie_self_knn");
}

extern "C" int jamie_lisi(const int32_t* idx, const float* dist, long long N, int K, const int32_t* codes, int n_sets,
                          double perplexity, double* lisi, int32_t* tries, void* stream) {
    JAMIE_ARG(idx && dist && codes && lisi, "null pointer");
    JAMIE_ARG(N >= 1 && K >= 2 && K <= SELF_KMAX, "N >= 1, 2 <= K <= 128");
    JAMIE_ARG(n_sets >= 1 && n_sets <= 4, "1 <= n_sets <= 4");
    JAMIE_ARG(perplexity > 1.0 && perplexity < (double)K, "1 < perplexity < K");
    hipLaunchKernelGGL(lisi_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, (hipStream_t)stream, idx, dist, N, K, codes, n_sets,
                       log(perplexity), lisi, tries);
    return jamie_launch_status("jamie_lisi");
}

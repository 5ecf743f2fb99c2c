// Alignment metrics on the device (include/jamie_hip.h "Alignment metrics on the device"; jamie_amd/metrics.py): FOSCTTM counts
// and a cross-set k-nearest-neighbour search + majority vote, all as streaming passes over the pair space of two [N, L] fp32
// embeddings.  Nothing of size N x N is stored.  The arithmetic of q, the pair tile, the running top-K of a wave and the
// neighbour-search workgroup are in pair_tile.h, shared with neighbors.hip.
#include "pair_tile.h"

namespace {

// own[i] = q(i, i): the chain of pair_tile on rows i of A and B
__global__ __launch_bounds__(256) void own_pair_kernel(const float* __restrict__ A, const float* __restrict__ B, long long N, int L,
                                                       float* __restrict__ own) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const float* a = A + i * L;
    const float* b = B + i * L;
    float q = 0.f;
    for (int c = 0; c < L; ++c) q = q_step(q, a[c], b[c]);
    own[i] = q;
}

// One workgroup: rows [i0, i0 + 128) of A against `walk` consecutive 128-row tiles of B.  Row counts stay in registers over the
// walk; column counts leave after every tile.  Integer adds only: LDS, then one global add per row (column) of the tile.
__global__ __launch_bounds__(256, 2) void foscttm_kernel(const float* __restrict__ A, const float* __restrict__ B, long long N,
                                                         int L, int vec, const float* __restrict__ own, long long tile_i0,
                                                         int walk, int* __restrict__ row_closer, int* __restrict__ col_closer) {
    __shared__ __attribute__((aligned(16))) float Xs[KC * LDJ];
    __shared__ __attribute__((aligned(16))) float Ys[KC * LDJ];
    __shared__ int rsum[128], csum[128];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const long long i0 = (tile_i0 + blockIdx.y) * 128;
    const long long ntj = (N + TJ - 1) / TJ;
    const long long jt0 = (long long)blockIdx.x * walk;
    const long long jt1 = jt0 + walk < ntj ? jt0 + walk : ntj;

    float di[8];
    int rc[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const long long gi = i0 + (r >> 2) * 64 + ty * 4 + (r & 3);
        di[r] = gi < N ? own[gi] : 0.f;
        rc[r] = 0;
    }
    if (threadIdx.x < 128) {
        rsum[threadIdx.x] = 0;
        csum[threadIdx.x] = 0;
    }
    for (long long jt = jt0; jt < jt1; ++jt) {
        const long long j0 = jt * TJ;
        float acc[8][8];
        pair_tile<2>(A, N, i0, B, N, j0, L, vec != 0, Xs, Ys, acc);
        float dj[8];
        int cc[8];
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const long long gj = j0 + (s >> 2) * 64 + tx * 4 + (s & 3);
            dj[s] = gj < N ? own[gj] : 0.f;
            cc[s] = 0;
        }
        if (i0 == j0 || i0 + 128 > N || j0 + TJ > N) {     // the tile holds own pairs (j = i) or runs past N: those never count
            const int ni = (int)(N - i0 < 128 ? N - i0 : 128), nj = (int)(N - j0 < TJ ? N - j0 : TJ);
            const int own_off = i0 == j0 ? 0 : 1 << 20;        // local row == local column + own_off: the cell's own pair
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int li = (r >> 2) * 64 + ty * 4 + (r & 3);
#pragma unroll
                for (int s = 0; s < 8; ++s) {
                    const int lj = (s >> 2) * 64 + tx * 4 + (s & 3);
                    if (li >= ni || lj >= nj || li == lj + own_off) acc[r][s] = __builtin_inff();
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 8; ++r)
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                rc[r] += acc[r][s] < di[r] ? 1 : 0;
                cc[s] += acc[r][s] < dj[s] ? 1 : 0;
            }
        // (csum was zeroed before the barriers inside pair_tile)
#pragma unroll
        for (int s = 0; s < 8; ++s) atomicAdd(&csum[(s >> 2) * 64 + tx * 4 + (s & 3)], cc[s]);
        __syncthreads();
        if (threadIdx.x < 128) {
            if (j0 + threadIdx.x < N) atomicAdd(&col_closer[j0 + threadIdx.x], csum[threadIdx.x]);
            csum[threadIdx.x] = 0;
        }
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) atomicAdd(&rsum[(r >> 2) * 64 + ty * 4 + (r & 3)], rc[r]);
    __syncthreads();
    if (threadIdx.x < 128 && i0 + threadIdx.x < N) atomicAdd(&row_closer[i0 + threadIdx.x], rsum[threadIdx.x]);
}

// a wave per query: the segments' lists offered in segment order, then idx and sqrt(q) out
__global__ __launch_bounds__(256) void knn_merge_kernel(const float* __restrict__ part_q, const int* __restrict__ part_i, long long Nq,
                                                        int K, int S, int32_t* __restrict__ idx, float* __restrict__ dist) {
    const int lane = threadIdx.x & 63;
    const long long gq = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gq >= Nq) return;
    float mq = __builtin_inff();
    int mi = 0x7fffffff;
    for (int s = 0; s < S; ++s) {
        const long long o = ((long long)s * Nq + gq) * K + lane;
        const bool valid = lane < K;
        const float cq = valid ? part_q[o] : 0.f;
        const int ci = valid ? part_i[o] : 0;
        wave_topk_offer(cq, ci, valid && ci != 0x7fffffff, K, mq, mi);
    }
    if (lane < K) {
        idx[gq * K + lane] = mi;
        dist[gq * K + lane] = sqrtf(mq);
    }
}

// pred[q] = the code most frequent among ref_codes[idx[q, :]], the lowest such code on a tie (K^2 compares: K <= 64)
__global__ __launch_bounds__(256) void knn_vote_kernel(const int32_t* __restrict__ idx, long long Nq, int K,
                                                       const int32_t* __restrict__ codes, int32_t* __restrict__ pred) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= Nq) return;
    const int32_t* row = idx + q * K;
    int best = 0x7fffffff, best_n = 0;
    for (int s = 0; s < K; ++s) {
        const int c = codes[row[s]];
        int n = 0;
        for (int t = 0; t < K; ++t) n += codes[row[t]] == c ? 1 : 0;
        if (n > best_n || (n == best_n && c < best)) {
            best = c;
            best_n = n;
        }
    }
    pred[q] = best;
}

}  // namespace

extern "C" long long jamie_metrics_workspace(long long Nq, long long Nr, int K) {
    if (Nq < 1 || Nr < 1 || K < 0) return 0;
    const long long own = Nq * 4;
    const long long lists = (long long)knn_segments(Nq, Nr, K) * Nq * K * 8;
    return own > lists ? own : lists;
}

extern "C" int jamie_foscttm_counts(const float* A, const float* B, long long N, int L, int32_t* row_closer, int32_t* col_closer,
                                    void* ws, long long ws_bytes, void* stream) {
    JAMIE_ARG(A && B && row_closer && col_closer && ws, "null pointer");
    JAMIE_ARG(N >= 1 && N < 2147483647ll && L >= 1, "1 <= N < 2^31, L >= 1");
    JAMIE_ARG(ws_bytes >= N * 4, "workspace smaller than jamie_metrics_workspace(N, N, 0)");
    hipStream_t st = (hipStream_t)stream;
    float* own = (float*)ws;
    const int vec = (L % 4 == 0) && aligned16(A) && aligned16(B);
    if (hipMemsetAsync(row_closer, 0, N * 4, st) != hipSuccess || hipMemsetAsync(col_closer, 0, N * 4, st) != hipSuccess)
        return jamie_launch_status("jamie_foscttm_counts");
    hipLaunchKernelGGL(own_pair_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, A, B, N, L, own);
    const long long nt = (N + 127) / 128;
    // tiles a workgroup walks: up to 8, fewer while that leaves the device short of workgroups
    int walk = (int)(nt * nt / 2048);
    walk = walk < 1 ? 1 : (walk > 8 ? 8 : walk);
    const long long step = tiles_per_launch(N, L, 128);
    for (long long t0 = 0; t0 < nt; t0 += step) {
        const long long n = nt - t0 < step ? nt - t0 : step;
        hipLaunchKernelGGL(foscttm_kernel, dim3((unsigned)((nt + walk - 1) / walk), (unsigned)n), dim3(256), 0, st, A, B, N, L, vec,
                           own, t0, walk, row_closer, col_closer);
    }
    return jamie_launch_status("jamie_foscttm_counts");
}

extern "C" int jamie_cross_knn(const float* Q, long long Nq, const float* R, long long Nr, int L, int K, int32_t* idx, float* dist,
                               void* ws, long long ws_bytes, void* stream) {
    JAMIE_ARG(K >= 1 && K <= KMAX && K <= Nr, "1 <= K <= min(Nr, 64)");
    JAMIE_ARG(Q && R && idx && dist && ws, "null pointer");
    JAMIE_ARG(Nq >= 1 && Nr >= 1 && Nr < 2147483647ll && L >= 1, "Nq, Nr, L >= 1, Nr < 2^31");
    JAMIE_ARG(ws_bytes >= jamie_metrics_workspace(Nq, Nr, K), "workspace smaller than jamie_metrics_workspace(Nq, Nr, K)");
    hipStream_t st = (hipStream_t)stream;
    const int S = knn_segments(Nq, Nr, K);
    const int QT = knn_query_tile(K);
    long long seg_len = (Nr + S - 1) / S;
    seg_len = (seg_len + TJ - 1) / TJ * TJ;
    float* part_q = (float*)ws;
    int* part_i = (int*)ws + (long long)S * Nq * K;
    const int vec = (L % 4 == 0) && aligned16(Q) && aligned16(R);
    const long long nt = (Nq + QT - 1) / QT;
    const long long step = tiles_per_launch(Nr, L, QT);
    for (long long t0 = 0; t0 < nt; t0 += step) {
        const long long n = nt - t0 < step ? nt - t0 : step;
        if (QT == 128)
            hipLaunchKernelGGL((knn_partial_kernel<2, K_SMALL, false, false>), dim3((unsigned)n, (unsigned)S), dim3(256), 0, st, Q, Nq,
                               R, Nr, L, vec, K, t0, seg_len, (const float*)nullptr, (const int*)nullptr, part_q, part_i);
        else
            hipLaunchKernelGGL((knn_partial_kernel<1, KMAX, false, false>), dim3((unsigned)n, (unsigned)S), dim3(256), 0, st, Q, Nq, R,
                               Nr, L, vec, K, t0, seg_len, (const float*)nullptr, (const int*)nullptr, part_q, part_i);
    }
    hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)((Nq + 3) / 4)), dim3(256), 0, st, part_q, part_i, Nq, K, S, idx, dist);
    return jamie_launch_status("jamie_cross_knn");
}

extern "C" int jamie_knn_vote(const int32_t* idx, long long Nq, int K, const int32_t* ref_codes, int n_classes, int32_t* pred,
                              void* stream) {
    JAMIE_ARG(idx && ref_codes && pred, "null pointer");
    JAMIE_ARG(Nq >= 1 && K >= 1 && n_classes >= 1, "Nq, K, n_classes >= 1");
    hipLaunchKernelGGL(knn_vote_kernel, dim3((unsigned)((Nq + 255) / 256)), dim3(256), 0, (hipStream_t)stream, idx, Nq, K, ref_codes,
                       pred);
    return jamie_launch_status("jamie_knn_vote");
}

// ---- silhouette widths: the pair space reduced to distance sums per (query row, class of the reference rows) ----
//
// R is sorted by class, so a class is a run of rows and a 128-row tile of it carries one class: the tile's sqrt(q) are added per
// row, first a thread's 8 columns in fp32 (ascending column order; 7 roundings at the scale of one tile row, so that the fp64
// adds that follow are one per 8 pairs and not one per pair: a v_add_f64 costs 4 issue slots of the loop's budget), then into 8
// fp64 row accumulators that stay in registers over the walk.  The order of every add is fixed by the thread's position in the
// workgroup and by the work list, never by timing: no atomics, equal bits from run to run, and a query row gets the same bits
// wherever it sits in Q (a row's columns are split over tx only).
namespace {

struct LabelWork {                // one workgroup's walk: rows [row0, row1) of one class, at most seg_tiles tiles
    long long row0, row1;
    long long out;                // direct: the class (column of S); else the partial slot
    long long direct;
};
struct LabelClass {               // the partial slots [slot0, slot0 + nslots) of a class, in segment order; nslots < 0: S written
    long long slot0, nslots;      // by the walk itself (one segment); nslots == 0: an empty class
};

// sqrt(q), q >= 0, in 8 issue slots where libm's correctly rounded sqrtf takes 23 (v_sqrt_f32, two candidates one ulp either side,
// compares, selects and their s_nops, a rescue of tiny q): r = v_sqrt_f32(q) is within one ulp, its residual e = q - r^2 is exact
// in one fma, and r + e / (2 r) with 1 / (2 r) from v_rsq_f32 (relative error 2^-22) is then rounded once: the Newton step leaves
// 2^-24 ulp, the error of 1 / (2 r) at most 2^-22 ulp of the correction, so the result is within (1/2 + 2^-21) ulp of sqrt(q):
// relative error u (1 + 2^-20), u = 2^-24.  q = 0 gives exactly 0 (e = 0, and the max keeps 1 / (2 r) finite).
// q below 2^-126 (a distance below 1e-19) is left to the hardware's handling of denormal operands; q = +inf (coordinates
// beyond 1e19) gives NaN where libm gives +inf.
__device__ __forceinline__ float dist_of_q(float q) {
    const float r = __builtin_amdgcn_sqrtf(q);
    const float h = 0.5f * __builtin_amdgcn_rsqf(fmaxf(q, 1.17549435e-38f));
    const float e = __builtin_fmaf(-r, r, q);
    return __builtin_fmaf(e, h, r);
}

__global__ __launch_bounds__(256, 2) void label_sums_kernel(const float* __restrict__ Q, long long Nq, const float* __restrict__ R,
                                                            int L, int vec, const LabelWork* __restrict__ work, long long tile_q0,
                                                            double* __restrict__ S, long long ldS, double* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float Xs[KC * LDJ];
    __shared__ __attribute__((aligned(16))) float Ys[KC * LDJ];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    // query tiles run fastest over the grid: the workgroups resident together walk the same few segments of R (from L2) and
    // differ in their 128 query rows
    const LabelWork w = work[blockIdx.y];
    const long long i0 = (tile_q0 + blockIdx.x) * 128;
    double sum[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) sum[r] = 0.0;
    for (long long j0 = w.row0; j0 < w.row1; j0 += TJ) {
        float acc[8][8];
        pair_tile<2>(Q, Nq, i0, R, w.row1, j0, L, vec != 0, Xs, Ys, acc);
        if (j0 + TJ > w.row1) {                            // the last tile of the class: columns past its end add sqrt(0) = 0
            const int nj = (int)(w.row1 - j0);
#pragma unroll
            for (int s = 0; s < 8; ++s)
                if ((s >> 2) * 64 + tx * 4 + (s & 3) >= nj) {
#pragma unroll
                    for (int r = 0; r < 8; ++r) acc[r][s] = 0.f;
                }
        }
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            float p = dist_of_q(acc[r][0]);
#pragma unroll
            for (int s = 1; s < 8; ++s) p += dist_of_q(acc[r][s]);
            sum[r] += (double)p;
        }
    }
    // the 16 tx lanes of a row are lanes ty % 4 * 16 + [0, 16) of one wave: a fixed xor tree (every lane ends with the same bits)
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        double v = sum[r];
        v += __shfl_xor(v, 8);
        v += __shfl_xor(v, 4);
        v += __shfl_xor(v, 2);
        v += __shfl_xor(v, 1);
        const long long gi = i0 + (r >> 2) * 64 + ty * 4 + (r & 3);
        if (tx == 0 && gi < Nq) {
            if (w.direct)
                S[gi * ldS + w.out] = v;
            else
                part[w.out * Nq + gi] = v;
        }
    }
}

// S[i, c] = the partials of class c added in segment order (0 for an empty class); classes the walk wrote are left alone
__global__ __launch_bounds__(256) void label_sums_finish_kernel(const double* __restrict__ part, const LabelClass* __restrict__ cls,
                                                                long long Nq, int C, double* __restrict__ S, long long ldS) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= Nq * C) return;
    const long long c = idx / Nq, i = idx - c * Nq;
    const LabelClass k = cls[c];
    if (k.nslots < 0) return;
    double v = 0.0;
    for (long long s = 0; s < k.nslots; ++s) v += part[(k.slot0 + s) * Nq + i];
    S[i * ldS + c] = v;
}

__global__ __launch_bounds__(256) void silhouette_kernel(const double* __restrict__ S, long long ldS, long long Nq,
                                                         const long long* __restrict__ counts, const int32_t* __restrict__ own,
                                                         const int32_t* __restrict__ win0, int wlen, double* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= Nq) return;
    const double nan = __builtin_nan("");
    const long long o = own[i];
    long long w0 = win0 ? win0[i] : 0;
    w0 = w0 < 0 ? 0 : w0;
    const long long w1 = w0 + wlen < ldS ? w0 + wlen : ldS;
    if (o < 0 || o >= ldS) {
        out[i] = nan;
        return;
    }
    const double* s = S + i * ldS;
    double b = 0.0;
    bool any = false;
    for (long long c = w0; c < w1; ++c) {
        const long long n = counts[c];
        if (c == o || n < 1) continue;
        const double m = s[c] / (double)n;
        b = (!any || m < b) ? m : b;
        any = true;
    }
    const long long n_own = counts[o];
    double v;
    if (!any) {
        v = nan;
    } else if (n_own <= 1) {
        v = 0.0;
    } else {
        const double a = s[o] / (double)(n_own - 1);
        const double mx = a > b ? a : b;
        v = mx == 0.0 ? 0.0 : (b - a) / mx;
    }
    out[i] = v;
}

// Tiles per segment when the caller leaves it to the library.  It depends on Nr alone, not on Nq: the queries may then be passed
// in chunks of any size and every row still gets the same bits.  About 64 segments over the whole of R keep the device busy under a
// single query tile (the neighbour search's reasoning: equally long workgroups, a few rounds of them); a segment keeps at least 8
// tiles and at most 64, so that the partials stay a few hundred fp64 per query row.
inline int label_seg_tiles(long long Nr, int seg_tiles) {
    if (seg_tiles > 0) return seg_tiles;
    const long long t = ((Nr + TJ - 1) / TJ + 63) / 64;
    return (int)(t < 8 ? 8 : (t > 64 ? 64 : t));
}
// sum over the classes of ceil(n_c / 128) is below this for any class sizes that add up to Nr
inline long long label_tiles_max(long long Nr, int C) { return Nr / TJ + (C < Nr ? C : Nr) + 1; }
inline long long label_items_max(long long Nr, int C, int seg) { return label_tiles_max(Nr, C) / seg + (C < Nr ? C : Nr) + 1; }
// partial slots: only classes of more than `seg` tiles have any (fewer than tiles / seg of them), ceil(t_c / seg) each
inline long long label_slots_max(long long Nr, int C, int seg) { return 2 * (label_tiles_max(Nr, C) / seg); }
inline long long label_head_bytes(long long Nr, int C, int seg) {
    const long long b = label_items_max(Nr, C, seg) * (long long)sizeof(LabelWork) + (long long)C * (long long)sizeof(LabelClass);
    return (b + 255) / 256 * 256;
}

}  // namespace

extern "C" long long jamie_label_sums_workspace(long long Nq, long long Nr, int C, int seg_tiles) {
    if (Nq < 1 || Nr < 1 || C < 1 || seg_tiles < 0) return 0;
    const int seg = label_seg_tiles(Nr, seg_tiles);
    return label_head_bytes(Nr, C, seg) + label_slots_max(Nr, C, seg) * Nq * 8;
}

extern "C" int jamie_label_distance_sums(const float* Q, long long Nq, const float* R, long long Nr, int L, const long long* class_off,
                                         int C, double* S, long long ldS, int seg_tiles, void* ws, long long ws_bytes, void* stream) {
    JAMIE_ARG(Q && R && class_off && S && ws, "null pointer");
    JAMIE_ARG(Nq >= 1 && Nr >= 1 && L >= 1 && C >= 1, "Nq, Nr, L, C >= 1");
    JAMIE_ARG(ldS >= C, "ldS >= C");
    JAMIE_ARG(seg_tiles >= 0, "seg_tiles >= 0");
    JAMIE_ARG(ws_bytes >= jamie_label_sums_workspace(Nq, Nr, C, seg_tiles),
              "workspace smaller than jamie_label_sums_workspace(Nq, Nr, C, seg_tiles)");
    hipStream_t st = (hipStream_t)stream;
    const int seg = label_seg_tiles(Nr, seg_tiles);
    // class_off is read back and checked here, and the work list is formed from it on the host: the call waits for the stream
    long long* off = (long long*)malloc(((size_t)C + 1) * sizeof(long long));
    const long long n_items_max = label_items_max(Nr, C, seg);
    const size_t head = (size_t)label_head_bytes(Nr, C, seg);
    char* host = (char*)malloc(head);
    if (!off || !host) {
        free(off);
        free(host);
        return jamie_fail(-2, "%s: out of host memory", "jamie_label_distance_sums");
    }
    if (hipMemcpyAsync(off, class_off, ((size_t)C + 1) * sizeof(long long), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
        free(off);
        free(host);
        return jamie_launch_status("jamie_label_distance_sums");
    }
    bool ok = off[0] == 0 && off[C] == Nr;
    for (int c = 0; c < C && ok; ++c) ok = off[c + 1] >= off[c];
    if (!ok) {
        free(off);
        free(host);
        return jamie_fail(-1, "%s: argument check failed: class_off must start at 0, not decrease and end at Nr [%lld %lld]",
                          "jamie_label_distance_sums", Nr, 0);
    }
    LabelWork* items = (LabelWork*)host;
    LabelClass* cls = (LabelClass*)(host + n_items_max * sizeof(LabelWork));
    long long n_items = 0, n_slots = 0;
    bool finish = false;
    for (int c = 0; c < C; ++c) {
        const long long tiles = (off[c + 1] - off[c] + TJ - 1) / TJ;
        const long long nseg = (tiles + seg - 1) / seg;
        cls[c].slot0 = n_slots;
        cls[c].nslots = nseg == 1 ? -1 : nseg;
        finish |= nseg != 1;
        for (long long s = 0; s < nseg; ++s) {
            LabelWork& w = items[n_items++];
            w.row0 = off[c] + s * seg * TJ;
            w.row1 = w.row0 + (long long)seg * TJ < off[c + 1] ? w.row0 + (long long)seg * TJ : off[c + 1];
            w.direct = nseg == 1;
            w.out = nseg == 1 ? c : n_slots++;
        }
    }
    free(off);
    const bool fits = n_items <= n_items_max && n_slots <= label_slots_max(Nr, C, seg);      // (the bounds above: always)
    if (!fits || hipMemcpyAsync(ws, host, head, hipMemcpyHostToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
        free(host);
        return fits ? jamie_launch_status("jamie_label_distance_sums")
                    : jamie_fail(-3, "%s: work list larger than its bound", "jamie_label_distance_sums");
    }
    free(host);
    const LabelWork* d_items = (const LabelWork*)ws;
    const LabelClass* d_cls = (const LabelClass*)((char*)ws + n_items_max * sizeof(LabelWork));
    double* part = (double*)((char*)ws + head);
    const int vec = (L % 4 == 0) && aligned16(Q) && aligned16(R);
    const long long nt = (Nq + 127) / 128;
    const long long step = tiles_per_launch(Nr, L, 128);
    for (long long t0 = 0; t0 < nt; t0 += step) {
        const long long n = nt - t0 < step ? nt - t0 : step;
        for (long long w0 = 0; w0 < n_items; w0 += 65535) {
            const long long nw = n_items - w0 < 65535 ? n_items - w0 : 65535;
            hipLaunchKernelGGL(label_sums_kernel, dim3((unsigned)n, (unsigned)nw), dim3(256), 0, st, Q, Nq, R, L, vec, d_items + w0, t0,
                               S, ldS, part);
        }
    }
    if (finish)
        hipLaunchKernelGGL(label_sums_finish_kernel, dim3((unsigned)((Nq * C + 255) / 256)), dim3(256), 0, st, part, d_cls, Nq, C, S,
                           ldS);
    return jamie_launch_status("jamie_label_distance_sums");
}

extern "C" int jamie_silhouette_widths(const double* S, long long ldS, long long Nq, const long long* counts, const int32_t* own,
                                       const int32_t* win0, int wlen, double* out, void* stream) {
    JAMIE_ARG(S && counts && own && out, "null pointer");
    JAMIE_ARG(Nq >= 1 && ldS >= 1 && wlen >= 1, "Nq, ldS, wlen >= 1");
    hipLaunchKernelGGL(silhouette_kernel, dim3((unsigned)((Nq + 255) / 256)), dim3(256), 0, (hipStream_t)stream, S, ldS, Nq, counts, own,
                       win0, wlen, out);
    return jamie_launch_status("jamie_silhouette_widths");
}

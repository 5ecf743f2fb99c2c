// Alignment metrics on the device (include/jamie_hip.h "Alignment metrics on the device"; jamie_amd/metrics.py): FOSCTTM counts
// and a cross-set k-nearest-neighbour search + majority vote, all as streaming passes over the pair space of two [N, L] fp32
// embeddings.  Nothing of size N x N is stored.
//
// Arithmetic: q(i, j) = sum_c (X[i, c] - Y[j, c])^2 by direct difference, one v_sub_f32 + one v_fma_f32 per pair and feature,
// accumulated in ascending c from 0 (`q_step`).  Every q in this file -- the pair tiles and the own-pair distances q(i, i) the
// FOSCTTM counts compare against -- is that one chain, so two q of the same operands are the same bits and both sides of
// `q(i, j) < q(i, i)` carry the same rounding.  Exact on integer-valued data.  Zero padding (features past L, rows past N) adds
// fma(0, 0, q) = q and changes nothing.
//
// Tile shape: 256 threads own TI x 128 pairs (TI = 128; 64 for a neighbour search with K > 16), a thread 8 x 8 (4 x 8) of them
// as two (one) groups of 4 rows x two groups of 4 columns.  Both operands are staged feature-major in LDS, 32 features at a time;
// per feature a thread reads its rows and columns as ds_read_b128 (rows: 4 addresses per wave, broadcast; columns: 16 contiguous
// 16-byte slots) and issues 128 (64) VALU instructions on them: the loop is bound by VALU issue, which needs the two workgroups
// per CU the launch bounds ask for (a lone wave on a SIMD issues v_fma_f32 every 4 cycles instead of every 2).
#include "common.h"

namespace {

constexpr int KC = 32;            // features staged per trip
constexpr int TJ = 128;           // columns (walked side) of a pair tile
constexpr int LDJ = TJ + 4;       // LDS row stride of the staged operands: +4 floats spreads the transposing writes over the banks
constexpr int KMAX = 64;          // neighbours per query: one list entry per lane of a wave
constexpr long long LAUNCH_WORK = 4000000000000ll;      // pair-features per launch (a fraction of a second)

__device__ __forceinline__ float q_step(float q, float a, float b) {
    const float t = a - b;
    return __builtin_fmaf(t, t, q);
}

// rows [r0, r0 + ROWS) x features [c0, c0 + KC) of M [n, L] -> S[feature][row], zero where the row or the feature does not exist
template <int ROWS>
__device__ __forceinline__ void stage(const float* __restrict__ M, long long n, long long r0, int L, int c0, bool vec,
                                      float* __restrict__ S) {
    constexpr int LD = ROWS + 4;
    for (int s = threadIdx.x; s < ROWS * (KC / 4); s += 256) {
        const int r = s >> 3, c = c0 + (s & 7) * 4;
        const long long gr = r0 + r;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (gr < n) {
            const float* p = M + gr * L + c;
            if (vec && c + 3 < L) {
                const float4 x = *reinterpret_cast<const float4*>(p);
                v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (c + k < L) v[k] = p[k];
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) S[((s & 7) * 4 + k) * LD + r] = v[k];
    }
}

// acc[r][s] = q(i0 + row(r), j0 + col(s)), row(r) = (r / 4) * 64 + ty * 4 + r % 4, col(s) = (s / 4) * 64 + tx * 4 + s % 4
template <int MI>
__device__ __forceinline__ void pair_tile(const float* __restrict__ X, long long nx, long long i0, const float* __restrict__ Y,
                                          long long ny, long long j0, int L, bool vec, float* Xs, float* Ys,
                                          float (&acc)[MI * 4][8]) {
    constexpr int LDI = MI * 64 + 4;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
#pragma unroll
    for (int r = 0; r < MI * 4; ++r)
#pragma unroll
        for (int s = 0; s < 8; ++s) acc[r][s] = 0.f;
    for (int c0 = 0; c0 < L; c0 += KC) {
        __syncthreads();                                   // the last trip's reads (or the caller's use of this LDS) are done
        stage<MI * 64>(X, nx, i0, L, c0, vec, Xs);
        stage<TJ>(Y, ny, j0, L, c0, vec, Ys);
        __syncthreads();
        const int rest = (L - c0 + 3) & ~3;
        const int kc = rest < KC ? rest : KC;
#pragma unroll 2
        for (int c = 0; c < kc; ++c) {
            float a[MI * 4], b[8];
#pragma unroll
            for (int m = 0; m < MI; ++m) {
                const float4 x = *reinterpret_cast<const float4*>(&Xs[c * LDI + m * 64 + ty * 4]);
                a[m * 4] = x.x; a[m * 4 + 1] = x.y; a[m * 4 + 2] = x.z; a[m * 4 + 3] = x.w;
            }
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const float4 y = *reinterpret_cast<const float4*>(&Ys[c * LDJ + m * 64 + tx * 4]);
                b[m * 4] = y.x; b[m * 4 + 1] = y.y; b[m * 4 + 2] = y.z; b[m * 4 + 3] = y.w;
            }
#pragma unroll
            for (int r = 0; r < MI * 4; ++r)
#pragma unroll
                for (int s = 0; s < 8; ++s) acc[r][s] = q_step(acc[r][s], a[r], b[s]);
        }
    }
}

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

// ---- running top-K of a wave: lane l holds the l-th smallest (q, index) seen so far, ascending by q, then by index ----
__device__ __forceinline__ bool key_less(float qa, int ia, float qb, int ib) { return qa < qb || (qa == qb && ia < ib); }

// The lane exchanges of an insertion are v_readlane_b32 (the source lane is the same for the whole wave) and one DPP wave shift:
// an insertion is a dependent chain, and the other waves of the workgroup wait at the barrier for it (with ds_bpermute, `__shfl`,
// in its place the N = 100 000, L = 32, k = 5 search took 21.0 instead of 20.0 ms).
__device__ __forceinline__ float lane_value(float v, int src) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), src));
}
__device__ __forceinline__ int lane_value(int v, int src) { return __builtin_amdgcn_readlane(v, src); }
__device__ __forceinline__ int from_lane_below(int v) {          // lane l <- lane l - 1 (lane 0 keeps its own): wave_shr:1
    return __builtin_amdgcn_update_dpp(v, v, 0x138, 0xF, 0xF, false);
}

// every lane offers one candidate (`valid`, cq, ci); those below the K-th entry are inserted, in lane order
__device__ __forceinline__ void wave_topk_offer(float cq, int ci, bool valid, int K, float& mq, int& mi) {
    const int lane = threadIdx.x & 63;
    float tq = lane_value(mq, K - 1);
    int ti = lane_value(mi, K - 1);
    unsigned long long todo = __ballot(valid && key_less(cq, ci, tq, ti));
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const float q = lane_value(cq, src);
        const int id = lane_value(ci, src);
        if (key_less(q, id, tq, ti)) {
            const int pos = __popcll(__ballot(key_less(mq, mi, q, id)));      // entries that stay in front (a prefix: sorted)
            const float uq = __builtin_bit_cast(float, from_lane_below(__builtin_bit_cast(int, mq)));
            const int ui = from_lane_below(mi);
            if (lane == pos) {
                mq = q;
                mi = id;
            } else if (lane > pos) {
                mq = uq;
                mi = ui;
            }
            tq = lane_value(mq, K - 1);
            ti = lane_value(mi, K - 1);
            todo &= __ballot(key_less(cq, ci, tq, ti));      // the K-th entry came down: most of the rest no longer qualify
        }
    }
}

constexpr int LDT = TJ + 4;       // row stride of the q tile in LDS

// One workgroup: MI * 64 queries against segment blockIdx.y of the reference rows, 128 at a time.  A wave owns the lists of a
// quarter of the queries, KP entries each, in LDS.  The q tile stays in registers unless a query has a candidate in it; then it
// goes to the selection through LDS (in the space of the staged operands), 64 queries at a time.  Two shapes: 128 queries with
// lists of 16 (the inner loop of the FOSCTTM kernel; K <= 16), 64 queries with lists of 64.
template <int MI, int KP>
__global__ __launch_bounds__(256, 2) void knn_partial_kernel(const float* __restrict__ Q, long long Nq, const float* __restrict__ R,
                                                             long long Nr, int L, int vec, int K, long long tile_q0,
                                                             long long seg_len, float* __restrict__ part_q,
                                                             int* __restrict__ part_i) {
    constexpr int QT = MI * 64;
    constexpr int STAGE = KC * (QT + 4) + KC * LDJ;
    constexpr int TILE = 64 * LDT;
    __shared__ __attribute__((aligned(16))) float smem[STAGE > TILE ? STAGE : TILE];
    __shared__ float lq[QT * KP];
    __shared__ int li[QT * KP];
    __shared__ unsigned rows_hit[2][MI * 2];               // bit (row % 32) of word row / 32, per tile parity
    float* Xs = smem;
    float* Ys = smem + KC * (QT + 4);
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long q0 = (tile_q0 + blockIdx.x) * QT;
    const long long r0 = (long long)blockIdx.y * seg_len;
    const long long r1 = r0 + seg_len < Nr ? r0 + seg_len : Nr;
    for (int s = threadIdx.x; s < QT * KP; s += 256) {
        lq[s] = __builtin_inff();
        li[s] = 0x7fffffff;
    }
    if (threadIdx.x < MI * 4) rows_hit[threadIdx.x / (MI * 2)][threadIdx.x % (MI * 2)] = 0;
    int parity = 0;
    for (long long j0 = r0; j0 < r1; j0 += TJ, parity ^= 1) {
        float acc[MI * 4][8];
        pair_tile<MI>(Q, Nq, q0, R, r1, j0, L, vec != 0, Xs, Ys, acc);
        // Which queries have a candidate in this tile at all?  Once the lists have settled almost none has: a thread tests its
        // values against the K-th entries of its queries (<=, and rows or columns that do not exist included: the selection
        // below decides exactly), the workgroup ORs the answers in LDS.
#pragma unroll
        for (int m = 0; m < MI; ++m) {
            unsigned hit = 0;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float tq = lq[(m * 64 + ty * 4 + r) * KP + K - 1];
                bool any = false;
#pragma unroll
                for (int s = 0; s < 8; ++s) any |= !(acc[m * 4 + r][s] > tq);
                hit |= any ? 1u << r : 0u;
            }
            if (hit) atomicOr(&rows_hit[parity][m * 2 + (ty >> 3)], hit << ((ty & 7) * 4));
        }
        __syncthreads();                                   // the staged operands are read: their space may take the q tile
        if (threadIdx.x < MI * 2) rows_hit[parity ^ 1][threadIdx.x] = 0;                 // (last read before this barrier)
        bool tile_in_lds = false;
#pragma unroll
        for (int h = 0; h < MI; ++h) {
            if ((rows_hit[parity][h * 2] | rows_hit[parity][h * 2 + 1]) == 0) continue;  // (the same answer in every thread)
            if (tile_in_lds) __syncthreads();
            tile_in_lds = true;
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int m = 0; m < 2; ++m)
                    *reinterpret_cast<float4*>(&smem[(ty * 4 + r) * LDT + m * 64 + tx * 4]) = make_float4(
                        acc[h * 4 + r][m * 4], acc[h * 4 + r][m * 4 + 1], acc[h * 4 + r][m * 4 + 2], acc[h * 4 + r][m * 4 + 3]);
            __syncthreads();
            const unsigned mine = (rows_hit[parity][h * 2 + (wave >> 1)] >> ((wave & 1) * 16)) & 0xffffu;
            for (unsigned todo = mine; todo; todo &= todo - 1) {
                const int trow = wave * 16 + __ffs((int)todo) - 1, row = h * 64 + trow;
                if (q0 + row >= Nq) break;
                const float tq = lq[row * KP + K - 1];
                const int ti = li[row * KP + K - 1];
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    const long long gj = j0 + m * 64 + lane;
                    float cq = smem[trow * LDT + m * 64 + lane];
                    cq = cq == cq ? cq : __builtin_inff();         // (inf - inf of huge finite inputs: last, not lost)
                    const bool valid = gj < r1;
                    if (__ballot(valid && key_less(cq, (int)gj, tq, ti))) {
                        float mq = lane < KP ? lq[row * KP + lane] : __builtin_inff();
                        int mi = lane < KP ? li[row * KP + lane] : 0x7fffffff;
                        wave_topk_offer(cq, (int)gj, valid, K, mq, mi);
                        if (lane < KP) {
                            lq[row * KP + lane] = mq;
                            li[row * KP + lane] = mi;
                        }
                    }
                }
            }
        }
    }
    __syncthreads();
    for (int row = wave; row < QT; row += 4) {
        const long long gq = q0 + row;
        if (gq < Nq && lane < K) {
            const long long o = ((long long)blockIdx.y * Nq + gq) * K + lane;
            part_q[o] = lq[row * KP + lane];
            part_i[o] = li[row * KP + lane];
        }
    }
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

// Segments the reference rows are split into.  A workgroup walks its whole segment, so the workgroups of a launch are long and
// equally long, and the device holds two per CU at a time: they run in rounds, and a last round that is nearly empty costs as much
// as a full one (782 query tiles on 256 CUs: 1.5 rounds).  More segments make the rounds shorter and the last one cheaper, but
// every segment fills its lists from empty, a few per cent of a pass each.  The count with the lowest estimate of both is taken;
// a segment keeps at least 8 tiles.
constexpr int K_SMALL = 16;       // up to here the neighbour search runs its 128-query shape
constexpr double SEGMENT_COST = 0.03;
inline int knn_query_tile(int K) { return K <= K_SMALL ? 128 : 64; }

int resident_workgroups() {
    static int slots = 0;
    if (!slots) {
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
            cus < 1)
            cus = 256;
        slots = 2 * cus;
    }
    return slots;
}

int knn_segments(long long Nq, long long Nr, int K) {
    const int QT = knn_query_tile(K);
    const long long qt = (Nq + QT - 1) / QT, rt = (Nr + TJ - 1) / TJ;
    const double slots = resident_workgroups();
    long long s_max = (rt + 7) / 8;
    s_max = s_max > 32 ? 32 : (s_max < 1 ? 1 : s_max);
    int best = 1;
    double best_cost = 0.0;
    for (int S = 1; S <= s_max; ++S) {
        const double rounds = (double)(qt * S) / slots;
        const double cost = (double)(long long)(rounds + 0.999999) / rounds + SEGMENT_COST * S;
        if (S == 1 || cost < best_cost) {
            best = S;
            best_cost = cost;
        }
    }
    return best;
}

long long tiles_per_launch(long long n_other, int L, int tile) {
    const long long per_tile = (long long)tile * n_other * (L > 0 ? L : 1);
    const long long t = LAUNCH_WORK / (per_tile > 0 ? per_tile : 1);
    return t < 1 ? 1 : (t > 65535 ? 65535 : t);
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

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
            hipLaunchKernelGGL((knn_partial_kernel<2, K_SMALL>), dim3((unsigned)n, (unsigned)S), dim3(256), 0, st, Q, Nq, R, Nr, L, vec,
                               K, t0, seg_len, part_q, part_i);
        else
            hipLaunchKernelGGL((knn_partial_kernel<1, KMAX>), dim3((unsigned)n, (unsigned)S), dim3(256), 0, st, Q, Nq, R, Nr, L, vec, K,
                               t0, seg_len, part_q, part_i);
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

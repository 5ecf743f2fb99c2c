// The pair-space machinery shared by csrc/metrics.hip (FOSCTTM, the cross search, the silhouette sums) and csrc/neighbors.hip (the
// self search): a TI x 128 tile of q by direct difference, the running top-K of a wave, and the neighbour-search workgroup.
//
// Arithmetic: q(i, j) = sum_c (X[i, c] - Y[j, c])^2 by direct difference, one v_sub_f32 + one v_fma_f32 per pair and feature,
// accumulated in ascending c from 0 (`q_step`).  Every q of both files -- the pair tiles and the own-pair distances q(i, i) the
// FOSCTTM counts compare against -- is that one chain, so two q of the same operands are the same bits and both sides of
// `q(i, j) < q(i, i)` carry the same rounding.  Exact on integer-valued data.  Zero padding (features past L, rows past N) adds
// fma(0, 0, q) = q and changes nothing.
//
// Tile shape: 256 threads own TI x 128 pairs (TI = 128; 64 for a neighbour search with K > 16), a thread 8 x 8 (4 x 8) of them
// as two (one) groups of 4 rows x two groups of 4 columns.  Both operands are staged feature-major in LDS, 32 features at a time;
// per feature a thread reads its rows and columns as ds_read_b128 (rows: 4 addresses per wave, broadcast; columns: 16 contiguous
// 16-byte slots) and issues 128 (64) VALU instructions on them: the loop is bound by VALU issue, which needs the two workgroups
// per CU the launch bounds ask for (a lone wave on a SIMD issues v_fma_f32 every 4 cycles instead of every 2).
#pragma once
#include "common.h"

namespace {

constexpr int KC = 32;            // features staged per trip
constexpr int TJ = 128;           // columns (walked side) of a pair tile
constexpr int LDJ = TJ + 4;       // LDS row stride of the staged operands: +4 floats spreads the transposing writes over the banks
constexpr int KMAX = 64;          // neighbours per list: one list entry per lane of a wave
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
//
// SELF: Q and R are the same rows and a query never takes itself, by index (`gj != gq`): a copy of it elsewhere is a neighbour
// at q = 0 like any other.  FLOOR: only candidates above the query's floor key (floor_q[gq], floor_i[gq]) in the order of
// `key_less` are admitted, in the selection and in the test for "a candidate at all": the second pass of a search for more
// neighbours than a list holds, the floor being the last entry of the first pass.
template <int MI, int KP, bool SELF, bool FLOOR>
__global__ __launch_bounds__(256, 2) void knn_partial_kernel(const float* __restrict__ Q, long long Nq, const float* __restrict__ R,
                                                             long long Nr, int L, int vec, int K, long long tile_q0,
                                                             long long seg_len, const float* __restrict__ floor_q,
                                                             const int* __restrict__ floor_i, float* __restrict__ part_q,
                                                             int* __restrict__ part_i) {
    constexpr int QT = MI * 64;
    constexpr int STAGE = KC * (QT + 4) + KC * LDJ;
    constexpr int TILE = 64 * LDT;
    __shared__ __attribute__((aligned(16))) float smem[STAGE > TILE ? STAGE : TILE];
    __shared__ float lq[QT * KP];
    __shared__ int li[QT * KP];
    __shared__ float fq_s[FLOOR ? QT : 1];
    __shared__ int fi_s[FLOOR ? QT : 1];
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
    if constexpr (FLOOR) {
        // (rows past Nq: a floor nothing is above; read after the first barrier inside pair_tile)
        if (threadIdx.x < QT) {
            const long long gq = q0 + threadIdx.x;
            fq_s[threadIdx.x] = gq < Nq ? floor_q[gq] : __builtin_inff();
            fi_s[threadIdx.x] = gq < Nq ? floor_i[gq] : 0x7fffffff;
        }
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
                if constexpr (FLOOR) {
                    const float fq = fq_s[m * 64 + ty * 4 + r];
#pragma unroll
                    for (int s = 0; s < 8; ++s) any |= !(acc[m * 4 + r][s] > tq) && !(acc[m * 4 + r][s] < fq);
                } else {
#pragma unroll
                    for (int s = 0; s < 8; ++s) any |= !(acc[m * 4 + r][s] > tq);
                }
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
                    bool valid = gj < r1;
                    if constexpr (SELF) valid = valid && gj != q0 + row;
                    if constexpr (FLOOR) valid = valid && key_less(fq_s[row], fi_s[row], cq, (int)gj);
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

// Segments the reference rows are split into.  A workgroup walks its whole segment, so the workgroups of a launch are long and
// equally long, and the device holds two per CU at a time: they run in rounds, and a last round that is nearly empty costs as much
// as a full one (782 query tiles on 256 CUs: 1.5 rounds).  More segments make the rounds shorter and the last one cheaper, but
// every segment fills its lists from empty, a few per cent of a pass each.  The count with the lowest estimate of both is taken;
// a segment keeps at least 8 tiles.
constexpr int K_SMALL = 16;       // up to here the neighbour search runs its 128-query shape
constexpr double SEGMENT_COST = 0.03;
inline int knn_query_tile(int K) { return K <= K_SMALL ? 128 : 64; }

inline int resident_workgroups() {
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

inline int knn_segments(long long Nq, long long Nr, int K) {
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

inline long long tiles_per_launch(long long n_other, int L, int tile) {
    const long long per_tile = (long long)tile * n_other * (L > 0 ? L : 1);
    const long long t = LAUNCH_WORK / (per_tile > 0 ? per_tile : 1);
    return t < 1 ? 1 : (t > 65535 ? 65535 : t);
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

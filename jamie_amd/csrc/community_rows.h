// The rows of a community sweep, shared by csrc/louvain.hip (the move phase) and csrc/leiden.hip (the refinement): the three bins of
// a node list, the open-addressing table a row's candidates are gathered in, the search for the best candidate, and the host side
// of a launch.  DESIGN.md §23 (the table, the bins), §24.
//
// A row of at most CR_SHORT_MAX entries is a wave's (four rows per workgroup, a table per wave in LDS), one of at most CR_LONG_MAX a
// workgroup's with its table in LDS, a longer one a workgroup's with its table in the workspace.  The table is keyed by an id with
// int64 sums: a compare-and-swap claims a slot, an integer add fills it, so the order of the atomics does not show; the best
// candidate is taken under the total order (gain descending, id ascending), so the order of the slots does not show either.
//
// What a sweep is about is its policy P, a struct around its graph `g` (rowptr, nnz, n and comm are read here) with a type Node and
//
//   bool admit(i, leave)                     whether node i is taken at all; if not, `leave` is written as its target
//   void gather(e, c, keys, sums, mask, acc) entry e of a row of community c: into the table and into the row's own sum `acc`
//   Node node(i, c, acc)                     what the offers of node i need beside its row
//   bool scans(nd)                           whether the candidates are looked at
//   void offer(nd, d, sum, best)             candidate d with its sum against the best so far
//   int  stay(i, c)                          the target of a node that nothing wins, and of one that is refused
//
// The kernels themselves, with their tables, stay in the two files: their names are what traces and DESIGN.md speak of.
#pragma once
#include "common.h"

namespace {

constexpr int CR_SHORT_MAX = 64;       // entries of a row a wave takes (jamie_amd/louvain.py SHORT_MAX)
constexpr int CR_LONG_MAX = 2048;      // entries of a row whose table fits LDS (jamie_amd/louvain.py LONG_MAX)
constexpr int CR_SHORT_SLOTS = 2 * CR_SHORT_MAX;
constexpr int CR_LONG_SLOTS = 2 * CR_LONG_MAX;
constexpr int CR_GROUP = 16;           // lanes per row of the kernels that only add a row up
constexpr long long CR_NODES_MAX = 1ll << 31;
constexpr long long CR_TWO_M_MAX = 1ll << 52;
constexpr int CR_FLAG_BIN = 1, CR_FLAG_COMM = 2, CR_FLAG_TABLE = 4;

inline long long cr_slots(long long len) {                   // (jamie_amd/louvain.py table_slots)
    long long s = 2;
    while (s < 2 * len + 2) s *= 2;
    return s;
}

__device__ __forceinline__ unsigned cr_hash(int c) {
    const unsigned x = (unsigned)c * 2654435761u;
    return x ^ (x >> 15);
}

// adds v to the slot of id d; the table holds at most half as many keys as it has slots
__device__ __forceinline__ void cr_table_add(int* keys, unsigned long long* sums, unsigned mask, int d, unsigned long long v) {
    unsigned h = cr_hash(d) & mask;
    for (unsigned tries = 0; tries <= mask; ++tries) {
        const int prev = atomicCAS(&keys[h], -1, d);
        if (prev == -1 || prev == d) {
            atomicAdd(&sums[h], v);
            return;
        }
        h = (h + 1) & mask;
    }
}

struct CrBest {
    double gain;
    int id;                                                  // -1: none
};

__device__ __forceinline__ bool cr_better(double g, int d, const CrBest& b) {
    return d >= 0 && (b.id < 0 || g > b.gain || (g == b.gain && d < b.id));
}

__device__ __forceinline__ long long cr_wave_sum(long long v) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);
    return v;
}

__device__ __forceinline__ CrBest cr_wave_best(CrBest b) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const double og = __shfl_xor(b.gain, s);
        const int od = __shfl_xor(b.id, s);
        if (cr_better(og, od, b)) {
            b.gain = og;
            b.id = od;
        }
    }
    return b;
}

// the extent of row i, clamped to the arrays
__device__ __forceinline__ void cr_row(const long long* __restrict__ rowptr, long long nnz, long long i, long long& e0, long long& e1) {
    e0 = rowptr[i];
    e1 = rowptr[i + 1];
    e0 = e0 < 0 ? 0 : e0;
    e1 = e1 > nnz ? nnz : e1;
    if (e1 < e0) e1 = e0;
}

// ---- 16 lanes per row ----
__device__ __forceinline__ long long cr_group_sum(long long v) {
#pragma unroll
    for (int s = CR_GROUP / 2; s > 0; s >>= 1) v += __shfl_xor(v, s);       // (every lane of the wave is here)
    return v;
}

// the row of this thread's group in a launch of 256 threads
__device__ __forceinline__ long long cr_group_row() { return (long long)blockIdx.x * (256 / CR_GROUP) + threadIdx.x / CR_GROUP; }

// the sum of f(e) over the entries of that row (0 past the last row), in every lane of the group
template <class F>
__device__ __forceinline__ long long cr_group_row_sum(const long long* __restrict__ rowptr, long long nnz, long long n, long long row,
                                                      F f) {
    long long acc = 0;
    if (row < n) {
        long long e0, e1;
        cr_row(rowptr, nnz, row, e0, e1);
        for (long long e = e0 + (threadIdx.x & (CR_GROUP - 1)); e < e1; e += CR_GROUP) acc += f(e);
    }
    return cr_group_sum(acc);
}

// ---- the three bins ----
// node i (in range) with its community and its row; false when the policy leaves it out, and, with the flag raised and the node
// left where it stays, when its community is out of range or its row longer than `limit`.  `writer`: the one lane that writes.
template <class P>
__device__ __forceinline__ bool cr_take(const P& p, int i, long long limit, bool writer, int& c, long long& e0, long long& e1,
                                        int32_t* __restrict__ target, int32_t* __restrict__ flag) {
    int leave = -1;
    if (!p.admit(i, leave)) {
        if (writer) target[i] = leave;
        return false;
    }
    c = p.g.comm[i];
    cr_row(p.g.rowptr, p.g.nnz, i, e0, e1);
    if (c < 0 || c >= p.g.n || e1 - e0 > limit) {
        if (writer) {
            atomicOr(flag, c < 0 || c >= p.g.n ? CR_FLAG_COMM : CR_FLAG_BIN);
            target[i] = p.stay(i, c);
        }
        return false;
    }
    return true;
}

// a wave per row, four rows per workgroup; (keys, sums): this wave's CR_SHORT_SLOTS slots in LDS.  Every wave reaches both barriers.
template <class P>
__device__ __forceinline__ void cr_short_rows(const P& p, const int32_t* __restrict__ nodes, long long count, int* keys,
                                              unsigned long long* sums, int32_t* __restrict__ target, int32_t* __restrict__ flag) {
    const int lane = threadIdx.x & 63;
    const long long at = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    int i = at < count ? nodes[at] : -1;                     // (the same in every lane of the wave, as everything it decides)
    if (i >= p.g.n) i = -1;
    int c = -1;
    long long e0 = 0, e1 = 0, acc = 0;
    if (i >= 0 && !cr_take(p, i, CR_SHORT_MAX, lane == 0, c, e0, e1, target, flag)) i = -1;
    if (i >= 0) {
#pragma unroll
        for (int t = lane; t < CR_SHORT_SLOTS; t += 64) {
            keys[t] = -1;
            sums[t] = 0;
        }
    }
    __syncthreads();
    if (i >= 0 && e0 + lane < e1) p.gather(e0 + lane, c, keys, sums, CR_SHORT_SLOTS - 1, acc);
    acc = cr_wave_sum(acc);
    __syncthreads();
    if (i < 0) return;
    const typename P::Node nd = p.node(i, c, acc);
    CrBest best = {0.0, -1};
    if (p.scans(nd)) {
#pragma unroll
        for (int t = lane; t < CR_SHORT_SLOTS; t += 64) {
            const int d = keys[t];
            if (d >= 0) p.offer(nd, d, (long long)sums[t], best);
        }
    }
    best = cr_wave_best(best);
    if (lane == 0) target[i] = best.id >= 0 ? best.id : p.stay(i, c);
}

// a workgroup's row with the table behind (keys, sums); GLOBAL: the table is in device memory, filled by atomics at the L2 and read
// back past the L1
template <bool GLOBAL, class P>
__device__ __forceinline__ void cr_block_row(const P& p, int i, int c, long long e0, long long e1, int* keys, unsigned long long* sums,
                                             unsigned mask, int32_t* __restrict__ target) {
    __shared__ long long red_acc[4];
    __shared__ double red_gain[4];
    __shared__ int red_id[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    long long acc = 0;
    for (long long e = e0 + threadIdx.x; e < e1; e += 256) p.gather(e, c, keys, sums, mask, acc);
    acc = cr_wave_sum(acc);
    if (lane == 0) red_acc[wv] = acc;
    if (GLOBAL) __threadfence();
    __syncthreads();
    acc = red_acc[0] + red_acc[1] + red_acc[2] + red_acc[3];
    const typename P::Node nd = p.node(i, c, acc);
    CrBest best = {0.0, -1};
    if (p.scans(nd)) {                                       // (the same in every thread of the workgroup)
        for (unsigned t = threadIdx.x; t <= mask; t += 256) {
            int d;
            unsigned long long s;
            if (GLOBAL) {
                d = __hip_atomic_load(&keys[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                s = __hip_atomic_load(&sums[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else {
                d = keys[t];
                s = sums[t];
            }
            if (d >= 0) p.offer(nd, d, (long long)s, best);
        }
    }
    best = cr_wave_best(best);
    if (lane == 0) {
        red_gain[wv] = best.gain;
        red_id[wv] = best.id;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int q = 1; q < 4; ++q)
            if (cr_better(red_gain[q], red_id[q], best)) {
                best.gain = red_gain[q];
                best.id = red_id[q];
            }
        target[i] = best.id >= 0 ? best.id : p.stay(i, c);
    }
}

// the node of this workgroup and its row; false (for the whole workgroup) when it is not taken
template <class P>
__device__ __forceinline__ bool cr_block_node(const P& p, const int32_t* __restrict__ nodes, long long limit, int& i, int& c,
                                              long long& e0, long long& e1, int32_t* __restrict__ target, int32_t* __restrict__ flag) {
    i = nodes[blockIdx.x];
    if (i < 0 || i >= p.g.n) return false;
    return cr_take(p, i, limit, threadIdx.x == 0, c, e0, e1, target, flag);
}

// a workgroup per row of at most CR_LONG_MAX entries; (keys, sums): CR_LONG_SLOTS slots in LDS
template <class P>
__device__ __forceinline__ void cr_long_row(const P& p, const int32_t* __restrict__ nodes, int* keys, unsigned long long* sums,
                                            int32_t* __restrict__ target, int32_t* __restrict__ flag) {
    int i, c;
    long long e0, e1;
    if (!cr_block_node(p, nodes, CR_LONG_MAX, i, c, e0, e1, target, flag)) return;
    for (int t = threadIdx.x; t < CR_LONG_SLOTS; t += 256) {
        keys[t] = -1;
        sums[t] = 0;
    }
    __syncthreads();
    cr_block_row<false>(p, i, c, e0, e1, keys, sums, CR_LONG_SLOTS - 1, target);
}

// a workgroup per longer row.  Row r of the list owns the slots [slot_off[r], slot_off[r + 1]) of the workspace: a power of two, at
// least 2 len + 2; the host has set the keys to -1 and the sums to 0
template <class P>
__device__ __forceinline__ void cr_global_row(const P& p, const int32_t* __restrict__ nodes, const long long* __restrict__ slot_off,
                                              long long n_slots, unsigned long long* sums, int* keys, int32_t* __restrict__ target,
                                              int32_t* __restrict__ flag) {
    int i, c;
    long long e0, e1;
    if (!cr_block_node(p, nodes, p.g.nnz, i, c, e0, e1, target, flag)) return;
    const long long s0 = slot_off[blockIdx.x], s1 = slot_off[blockIdx.x + 1], slots = s1 - s0;
    if (s0 < 0 || s1 > n_slots || slots < 2 * (e1 - e0) + 2 || slots > (1ll << 31) || (slots & (slots - 1)) != 0) {
        if (threadIdx.x == 0) {
            atomicOr(flag, CR_FLAG_TABLE);
            target[i] = p.stay(i, c);
        }
        return;
    }
    cr_block_row<true>(p, i, c, e0, e1, keys + s0, sums + s0, (unsigned)(slots - 1), target);
}

// ---- the host side of a launch over a node list ----
// `who`: the entry point, which has checked its pointers; g: its graph (n, nnz and gamma are read here); the three kernels of its bins
template <class G>
inline int cr_launch(const char* who, const G& g, long long two_m, const int32_t* nodes, long long n_short, long long n_long,
                     long long n_global, const long long* slot_off, long long n_slots, void* ws, long long ws_bytes, int32_t* target,
                     int32_t* flag, hipStream_t st, void (*short_kernel)(G, const int32_t*, long long, int32_t*, int32_t*),
                     void (*long_kernel)(G, const int32_t*, int32_t*, int32_t*),
                     void (*global_kernel)(G, const int32_t*, const long long*, long long, unsigned long long*, int*, int32_t*, int32_t*)) {
    JAMIE_ARG_AS(who, g.n >= 1 && g.n < CR_NODES_MAX && g.nnz >= 0, "1 <= n < 2^31, nnz >= 0");
    JAMIE_ARG_AS(who, two_m >= 1 && two_m < CR_TWO_M_MAX, "1 <= two_m < 2^52");
    JAMIE_ARG_AS(who, g.gamma > 0.0 && g.gamma <= 1.79e308, "gamma must be positive and finite");
    JAMIE_ARG_AS(who, n_short >= 0 && n_long >= 0 && n_global >= 0 && n_short + n_long + n_global <= g.n,
                 "the three counts are >= 0 and at most n in all");
    JAMIE_ARG_AS(who, n_global == 0 || (slot_off && ws && n_slots >= 1 && n_slots <= ws_bytes / 12 && ((uintptr_t)ws & 7) == 0),
                 "rows beyond the LDS cap need slot_off and an 8-byte aligned workspace of 12 n_slots bytes");
    if (n_short) hipLaunchKernelGGL(short_kernel, dim3((unsigned)((n_short + 3) / 4)), dim3(256), 0, st, g, nodes, n_short, target, flag);
    if (n_long) hipLaunchKernelGGL(long_kernel, dim3((unsigned)n_long), dim3(256), 0, st, g, nodes + n_short, target, flag);
    if (n_global) {
        unsigned long long* sums = (unsigned long long*)ws;
        int* keys = (int*)(sums + n_slots);
        if (hipMemsetAsync(sums, 0, (size_t)n_slots * 8, st) != hipSuccess || hipMemsetAsync(keys, 0xff, (size_t)n_slots * 4, st) != hipSuccess)
            return jamie_launch_status(who);
        hipLaunchKernelGGL(global_kernel, dim3((unsigned)n_global), dim3(256), 0, st, g, nodes + n_short + n_long, slot_off, n_slots, sums,
                           keys, target, flag);
    }
    return jamie_launch_status(who);
}

}  // namespace

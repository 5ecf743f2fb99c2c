// Leiden communities on the device (include/jamie_hip.h "Leiden communities on the device"; jamie_amd/leiden.py): the kernels of
// the refinement step of one level, on the integer CSR level graph of csrc/louvain.hip (rowptr int64, col int32, w int64) with the
// communities `comm` of the level's move phase.  DESIGN.md §24.
//
//   ld_cut_kernel            16 lanes per row: one integer add per row into cut[ref[i]]
//   ld_refine_short_kernel   a wave per row of at most 64 entries, four rows per workgroup, a 128-slot table per wave in LDS
//   ld_refine_long_kernel    a workgroup per row of at most 2048 entries, a 4096-slot table in LDS (48 KiB: three workgroups per CU)
//   ld_refine_global_kernel  a workgroup per longer row, its table in the workspace, sized from the row's length
//   ld_apply_kernel          a thread per node: ref, rtot, rsize and the merged and cancelled counts
//
// The bins, the node lists, the workspace and the open-addressing table (a compare-and-swap claims a slot, an integer add fills it)
// are those of csrc/louvain.hip, whose few table and reduction helpers are restated here so that file stays as it is; the table is
// keyed by the sub-community ref[j] and filled only from the entries inside the node's community.  Every sum is an integer sum, the
// two conditions and the gain are formed in fp64 in the one operation order of the definition, without contraction, and the best
// candidate is taken under the total order (gain descending, id ascending).  No floating-point atomics.  Bit-identical from run to
// run.
#include "common.h"

namespace {

constexpr int LD_SHORT_MAX = 64;       // entries of a row a wave takes (jamie_amd/louvain.py SHORT_MAX)
constexpr int LD_LONG_MAX = 2048;      // entries of a row whose table fits LDS (jamie_amd/louvain.py LONG_MAX)
constexpr int LD_SHORT_SLOTS = 2 * LD_SHORT_MAX;
constexpr int LD_LONG_SLOTS = 2 * LD_LONG_MAX;
constexpr int LD_GROUP = 16;           // lanes per row of the cut kernel
constexpr long long LD_NODES_MAX = 1ll << 31;
constexpr long long LD_TWO_M_MAX = 1ll << 52;
constexpr int LD_FLAG_BIN = 1, LD_FLAG_COMM = 2, LD_FLAG_TABLE = 4;

struct LdGraph {
    const long long* rowptr;
    const int32_t* col;
    const long long* w;
    long long nnz, n;
    const long long* k;
    const int32_t* comm;
    const long long* tot;
    const int32_t* ref;
    const long long* rtot;
    const int32_t* rsize;
    const long long* cut;
    double gamma, two_m;
};

__device__ __forceinline__ unsigned ld_hash(int c) {
    const unsigned x = (unsigned)c * 2654435761u;
    return x ^ (x >> 15);
}

// adds v to sub-community d's slot; the table holds at most half as many keys as it has slots
__device__ __forceinline__ void ld_table_add(int* keys, unsigned long long* sums, unsigned mask, int d, unsigned long long v) {
    unsigned h = ld_hash(d) & mask;
    for (unsigned tries = 0; tries <= mask; ++tries) {
        const int prev = atomicCAS(&keys[h], -1, d);
        if (prev == -1 || prev == d) {
            atomicAdd(&sums[h], v);
            return;
        }
        h = (h + 1) & mask;
    }
}

struct LdBest {
    double gain;
    int id;                                                  // -1: none
};

__device__ __forceinline__ bool ld_better(double g, int d, const LdBest& b) {
    return d >= 0 && (b.id < 0 || g > b.gain || (g == b.gain && d < b.id));
}

__device__ __forceinline__ long long ld_wave_sum(long long v) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);
    return v;
}

__device__ __forceinline__ LdBest ld_wave_best(LdBest b) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const double og = __shfl_xor(b.gain, s);
        const int od = __shfl_xor(b.id, s);
        if (ld_better(og, od, b)) {
            b.gain = og;
            b.id = od;
        }
    }
    return b;
}

// the extent of node i's row, clamped to the arrays
__device__ __forceinline__ void ld_row(const LdGraph& g, int i, long long& e0, long long& e1) {
    e0 = g.rowptr[i];
    e1 = g.rowptr[i + 1];
    e0 = e0 < 0 ? 0 : e0;
    e1 = e1 > g.nnz ? g.nnz : e1;
    if (e1 < e0) e1 = e0;
}

// wc(x, t): x >= gamma t (T - t) / two_m, the condition of a well-connected node or sub-community inside a community of total T
__device__ __forceinline__ bool ld_well(const LdGraph& g, long long x, long long t, long long T) {
#pragma clang fp contract(off)
    return (double)x >= ((g.gamma * (double)t) * (double)(T - t)) / g.two_m;
}

// whether node i (in range) still is alone in its sub-community
__device__ __forceinline__ bool ld_alone(const LdGraph& g, int i) {
    const int r = g.ref[i];
    return r == i && g.rsize[i] == 1;
}

// one entry of node i's row: inside the community c its weight goes to `inside` and into the table under its sub-community
__device__ __forceinline__ void ld_gather(const LdGraph& g, long long e, int c, int* keys, unsigned long long* sums, unsigned mask,
                                          long long& inside) {
    const long long j = g.col[e];
    if (j < 0 || j >= g.n || g.comm[j] != c) return;
    const long long we = g.w[e];
    const int s = g.ref[j];
    inside += we;
    if (s >= 0 && s < g.n) ld_table_add(keys, sums, mask, s, (unsigned long long)we);
}

// what a node needs beside its row
struct LdNode {
    int i;
    long long T;
    double gki;
};

__device__ __forceinline__ LdNode ld_node(const LdGraph& g, int i, int c) {
#pragma clang fp contract(off)
    LdNode nd;
    nd.i = i;
    nd.T = g.tot[c];
    nd.gki = g.gamma * (double)g.k[i];
    return nd;
}

__device__ __forceinline__ void ld_offer(const LdGraph& g, const LdNode& nd, int s, long long kis, LdBest& best) {
#pragma clang fp contract(off)
    if (s == nd.i) return;                                               // (an alone node has no entry of its own)
    const long long rt = g.rtot[s];
    if (s > nd.i && g.rsize[s] == 1) return;                             // the singleton rule
    if (!ld_well(g, g.cut[s], rt, nd.T)) return;
    const double gain = (double)kis - (nd.gki * (double)rt) / g.two_m;
    if (gain > 0.0 && ld_better(gain, s, best)) {
        best.gain = gain;
        best.id = s;
    }
}

__global__ __launch_bounds__(256) void ld_refine_short_kernel(LdGraph g, const int32_t* __restrict__ nodes, long long count,
                                                              int32_t* __restrict__ target, int32_t* __restrict__ flag) {
    __shared__ int keys[4][LD_SHORT_SLOTS];
    __shared__ unsigned long long sums[4][LD_SHORT_SLOTS];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long at = (long long)blockIdx.x * 4 + wv;
    int i = at < count ? nodes[at] : -1;                     // (the same in every lane of the wave, as everything it decides)
    if (i >= g.n) i = -1;
    int c = -1;
    long long e0 = 0, e1 = 0, inside = 0;
    if (i >= 0 && !ld_alone(g, i)) {                         // no longer alone: nothing to gather
        if (lane == 0) target[i] = g.ref[i];
        i = -1;
    }
    if (i >= 0) {
        c = g.comm[i];
        ld_row(g, i, e0, e1);
        if (c < 0 || c >= g.n || e1 - e0 > LD_SHORT_MAX) {
            if (lane == 0) {
                atomicOr(flag, c < 0 || c >= g.n ? LD_FLAG_COMM : LD_FLAG_BIN);
                target[i] = i;
            }
            i = -1;
        }
    }
    if (i >= 0) {
#pragma unroll
        for (int t = lane; t < LD_SHORT_SLOTS; t += 64) {
            keys[wv][t] = -1;
            sums[wv][t] = 0;
        }
    }
    __syncthreads();
    if (i >= 0 && e0 + lane < e1) ld_gather(g, e0 + lane, c, keys[wv], sums[wv], LD_SHORT_SLOTS - 1, inside);
    inside = ld_wave_sum(inside);
    __syncthreads();
    if (i < 0) return;
    const LdNode nd = ld_node(g, i, c);
    LdBest best = {0.0, -1};
    if (ld_well(g, inside, g.k[i], nd.T)) {
#pragma unroll
        for (int t = lane; t < LD_SHORT_SLOTS; t += 64) {
            const int s = keys[wv][t];
            if (s >= 0) ld_offer(g, nd, s, (long long)sums[wv][t], best);
        }
    }
    best = ld_wave_best(best);
    if (lane == 0) target[i] = best.id >= 0 ? best.id : i;
}

// a workgroup's row with the table behind (keys, sums); GLOBAL: the table is in device memory, filled by atomics at the L2 and read
// back past the L1
template <bool GLOBAL>
__device__ __forceinline__ void ld_refine_row(const LdGraph& g, int i, int c, long long e0, long long e1, int* keys,
                                              unsigned long long* sums, unsigned mask, int32_t* __restrict__ target) {
    __shared__ long long red_in[4];
    __shared__ double red_gain[4];
    __shared__ int red_id[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    long long inside = 0;
    for (long long e = e0 + threadIdx.x; e < e1; e += 256) ld_gather(g, e, c, keys, sums, mask, inside);
    inside = ld_wave_sum(inside);
    if (lane == 0) red_in[wv] = inside;
    if (GLOBAL) __threadfence();
    __syncthreads();
    inside = red_in[0] + red_in[1] + red_in[2] + red_in[3];
    const LdNode nd = ld_node(g, i, c);
    LdBest best = {0.0, -1};
    if (ld_well(g, inside, g.k[i], nd.T)) {                  // (the same in every thread of the workgroup)
        for (unsigned t = threadIdx.x; t <= mask; t += 256) {
            int s;
            unsigned long long v;
            if (GLOBAL) {
                s = __hip_atomic_load(&keys[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                v = __hip_atomic_load(&sums[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else {
                s = keys[t];
                v = sums[t];
            }
            if (s >= 0) ld_offer(g, nd, s, (long long)v, best);
        }
    }
    best = ld_wave_best(best);
    if (lane == 0) {
        red_gain[wv] = best.gain;
        red_id[wv] = best.id;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int q = 1; q < 4; ++q)
            if (ld_better(red_gain[q], red_id[q], best)) {
                best.gain = red_gain[q];
                best.id = red_id[q];
            }
        target[i] = best.id >= 0 ? best.id : i;
    }
}

// the node of this workgroup and its row; false when it is no longer alone (target = ref) or cannot be taken (with the flag raised
// and the node left where it is)
__device__ __forceinline__ bool ld_block_node(const LdGraph& g, const int32_t* __restrict__ nodes, long long limit, int& i, int& c,
                                              long long& e0, long long& e1, int32_t* __restrict__ target, int32_t* __restrict__ flag) {
    i = nodes[blockIdx.x];
    if (i < 0 || i >= g.n) return false;
    if (!ld_alone(g, i)) {
        if (threadIdx.x == 0) target[i] = g.ref[i];
        return false;
    }
    c = g.comm[i];
    ld_row(g, i, e0, e1);
    if (c < 0 || c >= g.n || e1 - e0 > limit) {
        if (threadIdx.x == 0) {
            atomicOr(flag, c < 0 || c >= g.n ? LD_FLAG_COMM : LD_FLAG_BIN);
            target[i] = i;
        }
        return false;
    }
    return true;
}

__global__ __launch_bounds__(256) void ld_refine_long_kernel(LdGraph g, const int32_t* __restrict__ nodes, int32_t* __restrict__ target,
                                                             int32_t* __restrict__ flag) {
    __shared__ int keys[LD_LONG_SLOTS];
    __shared__ unsigned long long sums[LD_LONG_SLOTS];
    int i, c;
    long long e0, e1;
    if (!ld_block_node(g, nodes, LD_LONG_MAX, i, c, e0, e1, target, flag)) return;       // (the whole workgroup)
    for (int t = threadIdx.x; t < LD_LONG_SLOTS; t += 256) {
        keys[t] = -1;
        sums[t] = 0;
    }
    __syncthreads();
    ld_refine_row<false>(g, i, c, e0, e1, keys, sums, LD_LONG_SLOTS - 1, target);
}

// row r of the list owns the slots [slot_off[r], slot_off[r + 1]) of the workspace: a power of two, at least 2 len + 2; the host
// has set the keys to -1 and the sums to 0
__global__ __launch_bounds__(256) void ld_refine_global_kernel(LdGraph g, const int32_t* __restrict__ nodes,
                                                               const long long* __restrict__ slot_off, long long n_slots,
                                                               unsigned long long* sums, int* keys, int32_t* __restrict__ target,
                                                               int32_t* __restrict__ flag) {
    int i, c;
    long long e0, e1;
    if (!ld_block_node(g, nodes, g.nnz, i, c, e0, e1, target, flag)) return;             // (the whole workgroup)
    const long long s0 = slot_off[blockIdx.x], s1 = slot_off[blockIdx.x + 1], slots = s1 - s0;
    if (s0 < 0 || s1 > n_slots || slots < 2 * (e1 - e0) + 2 || slots > (1ll << 31) || (slots & (slots - 1)) != 0) {
        if (threadIdx.x == 0) {
            atomicOr(flag, LD_FLAG_TABLE);
            target[i] = i;
        }
        return;
    }
    ld_refine_row<true>(g, i, c, e0, e1, keys + s0, sums + s0, (unsigned)(slots - 1), target);
}

__global__ __launch_bounds__(256) void ld_cut_kernel(const long long* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                     const long long* __restrict__ w, long long nnz, long long n,
                                                     const int32_t* __restrict__ comm, const int32_t* __restrict__ ref,
                                                     unsigned long long* __restrict__ cut) {
    const int l = threadIdx.x & (LD_GROUP - 1);
    const long long row = (long long)blockIdx.x * (256 / LD_GROUP) + threadIdx.x / LD_GROUP;
    long long acc = 0;
    int s = -1;
    if (row < n) {
        const int c = comm[row];
        s = ref[row];
        long long e0 = rowptr[row], e1 = rowptr[row + 1];
        e0 = e0 < 0 ? 0 : e0;
        e1 = e1 > nnz ? nnz : e1;
        for (long long e = e0 + l; e < e1; e += LD_GROUP) {
            const long long j = col[e];
            if (j >= 0 && j < n && comm[j] == c && ref[j] != s) acc += w[e];
        }
    }
#pragma unroll
    for (int t = LD_GROUP / 2; t > 0; t >>= 1) acc += __shfl_xor(acc, t);       // (every lane of the wave is here)
    if (row < n && l == 0 && acc != 0 && s >= 0 && s < n) atomicAdd(&cut[s], (unsigned long long)acc);
}

__global__ __launch_bounds__(256) void ld_apply_kernel(const int32_t* __restrict__ nodes, long long count,
                                                       const int32_t* __restrict__ target, const long long* __restrict__ k,
                                                       int32_t* __restrict__ ref, unsigned long long* __restrict__ rtot,
                                                       int32_t* __restrict__ rsize, unsigned long long* __restrict__ counts, long long n) {
    const long long at = (long long)blockIdx.x * 256 + threadIdx.x;
    long long merged = 0, cancelled = 0;
    if (at < count) {
        const int i = nodes[at];
        if (i >= 0 && i < n) {
            const int r = ref[i], s = target[i];
            if (s != r && s >= 0 && s < n && r >= 0 && r < n) {
                if (target[s] != s) {
                    cancelled = 1;                             // s's founder is itself leaving in this sub-sweep
                } else {
                    const unsigned long long ki = (unsigned long long)k[i];
                    ref[i] = s;
                    atomicAdd(&rtot[r], 0ull - ki);            // (two's complement: rtot_r -= k_i)
                    atomicAdd(&rtot[s], ki);
                    atomicAdd(&rsize[r], -1);
                    atomicAdd(&rsize[s], 1);
                    merged = 1;
                }
            }
        }
    }
    merged = ld_wave_sum(merged);
    cancelled = ld_wave_sum(cancelled);
    if ((threadIdx.x & 63) == 0) {
        if (merged) atomicAdd(&counts[0], (unsigned long long)merged);
        if (cancelled) atomicAdd(&counts[1], (unsigned long long)cancelled);
    }
}

}  // namespace

extern "C" int jamie_leiden_cut(const long long* rowptr, const int32_t* col, const long long* w, long long nnz, long long n,
                                const int32_t* comm, const int32_t* ref, long long* cut, void* stream) {
    JAMIE_ARG(rowptr && comm && ref && cut && (nnz == 0 || (col && w)), "null pointer");
    JAMIE_ARG(n >= 1 && n < LD_NODES_MAX && nnz >= 0, "1 <= n < 2^31, nnz >= 0");
    hipLaunchKernelGGL(ld_cut_kernel, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, (hipStream_t)stream, rowptr, col, w, nnz, n, comm, ref,
                       (unsigned long long*)cut);
    return jamie_launch_status("jamie_leiden_cut");
}

extern "C" int jamie_leiden_refine(const long long* rowptr, const int32_t* col, const long long* w, long long nnz, long long n,
                                   const long long* k, const int32_t* comm, const long long* tot, const int32_t* ref,
                                   const long long* rtot, const int32_t* rsize, const long long* cut, double gamma, long long two_m,
                                   const int32_t* nodes, long long n_short, long long n_long, long long n_global,
                                   const long long* slot_off, long long n_slots, void* ws, long long ws_bytes, int32_t* target,
                                   int32_t* flag, void* stream) {
    JAMIE_ARG(rowptr && k && comm && tot && ref && rtot && rsize && cut && nodes && target && flag && (nnz == 0 || (col && w)),
              "null pointer");
    JAMIE_ARG(n >= 1 && n < LD_NODES_MAX && nnz >= 0, "1 <= n < 2^31, nnz >= 0");
    JAMIE_ARG(two_m >= 1 && two_m < LD_TWO_M_MAX, "1 <= two_m < 2^52");
    JAMIE_ARG(gamma > 0.0 && gamma <= 1.79e308, "gamma must be positive and finite");
    JAMIE_ARG(n_short >= 0 && n_long >= 0 && n_global >= 0 && n_short + n_long + n_global <= n, "the three counts are >= 0 and at most n in all");
    JAMIE_ARG((const void*)target != (const void*)ref && (const void*)target != (const void*)comm, "target must differ from ref and comm");
    JAMIE_ARG(n_global == 0 || (slot_off && ws && n_slots >= 1 && n_slots <= ws_bytes / 12 && ((uintptr_t)ws & 7) == 0),
              "rows beyond the LDS cap need slot_off and an 8-byte aligned workspace of 12 n_slots bytes");
    hipStream_t st = (hipStream_t)stream;
    const LdGraph g = {rowptr, col, w, nnz, n, k, comm, tot, ref, rtot, rsize, cut, gamma, (double)two_m};
    if (n_short)
        hipLaunchKernelGGL(ld_refine_short_kernel, dim3((unsigned)((n_short + 3) / 4)), dim3(256), 0, st, g, nodes, n_short, target, flag);
    if (n_long)
        hipLaunchKernelGGL(ld_refine_long_kernel, dim3((unsigned)n_long), dim3(256), 0, st, g, nodes + n_short, target, flag);
    if (n_global) {
        unsigned long long* sums = (unsigned long long*)ws;
        int* keys = (int*)(sums + n_slots);
        if (hipMemsetAsync(sums, 0, (size_t)n_slots * 8, st) != hipSuccess || hipMemsetAsync(keys, 0xff, (size_t)n_slots * 4, st) != hipSuccess)
            return jamie_launch_status("jamie_leiden_refine");
        hipLaunchKernelGGL(ld_refine_global_kernel, dim3((unsigned)n_global), dim3(256), 0, st, g, nodes + n_short + n_long, slot_off,
                           n_slots, sums, keys, target, flag);
    }
    return jamie_launch_status("jamie_leiden_refine");
}

extern "C" int jamie_leiden_apply(const int32_t* nodes, long long count, const int32_t* target, const long long* k, int32_t* ref,
                                  long long* rtot, int32_t* rsize, long long* counts, long long n, void* stream) {
    JAMIE_ARG(nodes && target && k && ref && rtot && rsize && counts, "null pointer");
    JAMIE_ARG(n >= 1 && n < LD_NODES_MAX && count >= 1 && count <= n, "1 <= count <= n < 2^31");
    JAMIE_ARG((const void*)target != (const void*)ref, "target must differ from ref");
    hipLaunchKernelGGL(ld_apply_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, (hipStream_t)stream, nodes, count, target, k,
                       ref, (unsigned long long*)rtot, rsize, (unsigned long long*)counts, n);
    return jamie_launch_status("jamie_leiden_apply");
}

// Louvain communities on the device (include/jamie_hip.h "Louvain communities on the device"; jamie_amd/louvain.py): the kernels
// of one level of modularity optimisation on an integer CSR level graph (rowptr int64, col int32, w int64, loop int64).  DESIGN.md
// §23.
//
//   lv_quantise_kernel     16 lanes per row: w_e = max(1, rint(val_e 2^20)), k_i = the row's sum
//   lv_move_short_kernel   a wave per row of at most 64 entries, four rows per workgroup, a 128-slot table per wave in LDS
//   lv_move_long_kernel    a workgroup per row of at most 2048 entries, a 4096-slot table in LDS (48 KiB: three workgroups per CU)
//   lv_move_global_kernel  a workgroup per longer row, its table in the workspace, sized from the row's length
//   lv_apply_kernel        a thread per node: comm, tot, size and the moved count
//   lv_internal_kernel     16 lanes per row: in_c
//
// A row's candidates are gathered in an open-addressing table keyed by community id with int64 sums (a compare-and-swap claims a
// slot, an integer add fills it), the node's own community aside in a register.  Every sum is an integer sum, so the order of
// the atomics does not show; the best candidate is taken under the total order (gain descending, id ascending), so the order of
// the slots does not show either.  The gain is formed in fp64 in the one operation order of the definition, without contraction.
// No floating-point atomics.  Bit-identical from run to run.
#include "common.h"

namespace {

constexpr int LV_SHORT_MAX = 64;       // entries of a row a wave takes (jamie_amd/louvain.py SHORT_MAX)
constexpr int LV_LONG_MAX = 2048;      // entries of a row whose table fits LDS (jamie_amd/louvain.py LONG_MAX)
constexpr int LV_SHORT_SLOTS = 2 * LV_SHORT_MAX;
constexpr int LV_LONG_SLOTS = 2 * LV_LONG_MAX;
constexpr int LV_GROUP = 16;           // lanes per row of the quantise and internal kernels
constexpr long long LV_NODES_MAX = 1ll << 31;
constexpr long long LV_TWO_M_MAX = 1ll << 52;
constexpr int LV_FLAG_BIN = 1, LV_FLAG_COMM = 2, LV_FLAG_TABLE = 4;

struct LvGraph {
    const long long* rowptr;
    const int32_t* col;
    const long long* w;
    long long nnz, n;
    const long long* k;
    const int32_t* comm;
    const long long* tot;
    const int32_t* size;
    double gamma, two_m;
};

inline long long lv_slots(long long len) {                   // (jamie_amd/louvain.py table_slots)
    long long s = 2;
    while (s < 2 * len + 2) s *= 2;
    return s;
}

__device__ __forceinline__ unsigned lv_hash(int c) {
    const unsigned x = (unsigned)c * 2654435761u;
    return x ^ (x >> 15);
}

// adds v to community d's slot; the table holds at most half as many keys as it has slots
__device__ __forceinline__ void lv_table_add(int* keys, unsigned long long* sums, unsigned mask, int d, unsigned long long v) {
    unsigned h = lv_hash(d) & mask;
    for (unsigned tries = 0; tries <= mask; ++tries) {
        const int prev = atomicCAS(&keys[h], -1, d);
        if (prev == -1 || prev == d) {
            atomicAdd(&sums[h], v);
            return;
        }
        h = (h + 1) & mask;
    }
}

struct LvBest {
    double gain;
    int id;                                                  // -1: none
};

__device__ __forceinline__ bool lv_better(double g, int d, const LvBest& b) {
    return d >= 0 && (b.id < 0 || g > b.gain || (g == b.gain && d < b.id));
}

// what a node needs beside its row
struct LvNode {
    int c;
    bool single;
    double gki, gain_c;
};

__device__ __forceinline__ double lv_gain(long long kid, double gki, long long T, double two_m) {
#pragma clang fp contract(off)
    return (double)kid - (gki * (double)T) / two_m;
}

__device__ __forceinline__ void lv_offer(const LvGraph& g, const LvNode& nd, int d, long long kid, LvBest& best) {
    if (nd.single && d > nd.c && g.size[d] == 1) return;      // the singleton rule
    const double gain = lv_gain(kid, nd.gki, g.tot[d], g.two_m);
    if (gain > nd.gain_c && lv_better(gain, d, best)) {
        best.gain = gain;
        best.id = d;
    }
}

__device__ __forceinline__ long long lv_wave_sum(long long v) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);
    return v;
}

__device__ __forceinline__ LvBest lv_wave_best(LvBest b) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const double og = __shfl_xor(b.gain, s);
        const int od = __shfl_xor(b.id, s);
        if (lv_better(og, od, b)) {
            b.gain = og;
            b.id = od;
        }
    }
    return b;
}

// the extent of node i's row, clamped to the arrays
__device__ __forceinline__ void lv_row(const LvGraph& g, int i, long long& e0, long long& e1) {
    e0 = g.rowptr[i];
    e1 = g.rowptr[i + 1];
    e0 = e0 < 0 ? 0 : e0;
    e1 = e1 > g.nnz ? g.nnz : e1;
    if (e1 < e0) e1 = e0;
}

// one entry of node i's row: its weight goes to `own` or into the table
__device__ __forceinline__ void lv_gather(const LvGraph& g, long long e, int c, int* keys, unsigned long long* sums, unsigned mask,
                                          long long& own) {
    const long long j = g.col[e];
    if (j < 0 || j >= g.n) return;
    const int d = g.comm[j];
    const long long we = g.w[e];
    if (d == c) own += we;
    else if (d >= 0 && d < g.n) lv_table_add(keys, sums, mask, d, (unsigned long long)we);
}

__device__ __forceinline__ LvNode lv_node(const LvGraph& g, int i, int c, long long own) {
#pragma clang fp contract(off)
    LvNode nd;
    const long long ki = g.k[i];
    nd.c = c;
    nd.single = g.size[c] == 1;
    nd.gki = g.gamma * (double)ki;
    nd.gain_c = lv_gain(own, nd.gki, g.tot[c] - ki, g.two_m);
    return nd;
}

__global__ __launch_bounds__(256) void lv_move_short_kernel(LvGraph g, const int32_t* __restrict__ nodes, long long count,
                                                            int32_t* __restrict__ target, int32_t* __restrict__ flag) {
    __shared__ int keys[4][LV_SHORT_SLOTS];
    __shared__ unsigned long long sums[4][LV_SHORT_SLOTS];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long at = (long long)blockIdx.x * 4 + wv;
#pragma unroll
    for (int t = lane; t < LV_SHORT_SLOTS; t += 64) {
        keys[wv][t] = -1;
        sums[wv][t] = 0;
    }
    __syncthreads();
    int i = at < count ? nodes[at] : -1;                     // (the same in every lane of the wave, as everything it decides)
    if (i >= g.n) i = -1;
    int c = -1;
    long long e0 = 0, e1 = 0, own = 0;
    if (i >= 0) {
        c = g.comm[i];
        lv_row(g, i, e0, e1);
        if (c < 0 || c >= g.n || e1 - e0 > LV_SHORT_MAX) {
            if (lane == 0) {
                atomicOr(flag, c < 0 || c >= g.n ? LV_FLAG_COMM : LV_FLAG_BIN);
                target[i] = c;
            }
            i = -1;
        }
    }
    if (i >= 0 && e0 + lane < e1) lv_gather(g, e0 + lane, c, keys[wv], sums[wv], LV_SHORT_SLOTS - 1, own);
    own = lv_wave_sum(own);
    __syncthreads();
    if (i < 0) return;
    const LvNode nd = lv_node(g, i, c, own);
    LvBest best = {0.0, -1};
#pragma unroll
    for (int t = lane; t < LV_SHORT_SLOTS; t += 64) {
        const int d = keys[wv][t];
        if (d >= 0) lv_offer(g, nd, d, (long long)sums[wv][t], best);
    }
    best = lv_wave_best(best);
    if (lane == 0) target[i] = best.id >= 0 ? best.id : c;
}

// a workgroup's row with the table behind (keys, sums); GLOBAL: the table is in device memory, filled by atomics at the L2 and read
// back past the L1
template <bool GLOBAL>
__device__ __forceinline__ void lv_move_row(const LvGraph& g, int i, int c, long long e0, long long e1, int* keys,
                                            unsigned long long* sums, unsigned mask, int32_t* __restrict__ target) {
    __shared__ long long red_own[4];
    __shared__ double red_gain[4];
    __shared__ int red_id[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    long long own = 0;
    for (long long e = e0 + threadIdx.x; e < e1; e += 256) lv_gather(g, e, c, keys, sums, mask, own);
    own = lv_wave_sum(own);
    if (lane == 0) red_own[wv] = own;
    if (GLOBAL) __threadfence();
    __syncthreads();
    own = red_own[0] + red_own[1] + red_own[2] + red_own[3];
    const LvNode nd = lv_node(g, i, c, own);
    LvBest best = {0.0, -1};
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
        if (d >= 0) lv_offer(g, nd, d, (long long)s, best);
    }
    best = lv_wave_best(best);
    if (lane == 0) {
        red_gain[wv] = best.gain;
        red_id[wv] = best.id;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int q = 1; q < 4; ++q)
            if (lv_better(red_gain[q], red_id[q], best)) {
                best.gain = red_gain[q];
                best.id = red_id[q];
            }
        target[i] = best.id >= 0 ? best.id : c;
    }
}

// the node of this workgroup and its row; false (with the flag raised and the node left where it is) when it cannot be taken
__device__ __forceinline__ bool lv_block_node(const LvGraph& g, const int32_t* __restrict__ nodes, long long limit, int& i, int& c,
                                              long long& e0, long long& e1, int32_t* __restrict__ target, int32_t* __restrict__ flag) {
    i = nodes[blockIdx.x];
    if (i < 0 || i >= g.n) return false;
    c = g.comm[i];
    lv_row(g, i, e0, e1);
    if (c < 0 || c >= g.n || e1 - e0 > limit) {
        if (threadIdx.x == 0) {
            atomicOr(flag, c < 0 || c >= g.n ? LV_FLAG_COMM : LV_FLAG_BIN);
            target[i] = c;
        }
        return false;
    }
    return true;
}

__global__ __launch_bounds__(256) void lv_move_long_kernel(LvGraph g, const int32_t* __restrict__ nodes, int32_t* __restrict__ target,
                                                           int32_t* __restrict__ flag) {
    __shared__ int keys[LV_LONG_SLOTS];
    __shared__ unsigned long long sums[LV_LONG_SLOTS];
    int i, c;
    long long e0, e1;
    if (!lv_block_node(g, nodes, LV_LONG_MAX, i, c, e0, e1, target, flag)) return;       // (the whole workgroup)
    for (int t = threadIdx.x; t < LV_LONG_SLOTS; t += 256) {
        keys[t] = -1;
        sums[t] = 0;
    }
    __syncthreads();
    lv_move_row<false>(g, i, c, e0, e1, keys, sums, LV_LONG_SLOTS - 1, target);
}

// row r of the list owns the slots [slot_off[r], slot_off[r + 1]) of the workspace: a power of two, at least 2 len + 2; the host
// has set the keys to -1 and the sums to 0
__global__ __launch_bounds__(256) void lv_move_global_kernel(LvGraph g, const int32_t* __restrict__ nodes,
                                                             const long long* __restrict__ slot_off, long long n_slots,
                                                             unsigned long long* sums, int* keys, int32_t* __restrict__ target,
                                                             int32_t* __restrict__ flag) {
    int i, c;
    long long e0, e1;
    if (!lv_block_node(g, nodes, g.nnz, i, c, e0, e1, target, flag)) return;             // (the whole workgroup)
    const long long s0 = slot_off[blockIdx.x], s1 = slot_off[blockIdx.x + 1], slots = s1 - s0;
    if (s0 < 0 || s1 > n_slots || slots < 2 * (e1 - e0) + 2 || slots > (1ll << 31) || (slots & (slots - 1)) != 0) {
        if (threadIdx.x == 0) {
            atomicOr(flag, LV_FLAG_TABLE);
            target[i] = c;
        }
        return;
    }
    lv_move_row<true>(g, i, c, e0, e1, keys + s0, sums + s0, (unsigned)(slots - 1), target);
}

__global__ __launch_bounds__(256) void lv_apply_kernel(const int32_t* __restrict__ nodes, long long count,
                                                       const int32_t* __restrict__ target, const long long* __restrict__ k,
                                                       int32_t* __restrict__ comm, unsigned long long* __restrict__ tot,
                                                       int32_t* __restrict__ size, unsigned long long* __restrict__ moved, long long n) {
    const long long at = (long long)blockIdx.x * 256 + threadIdx.x;
    long long one = 0;
    if (at < count) {
        const int i = nodes[at];
        if (i >= 0 && i < n) {
            const int c = comm[i], d = target[i];
            if (d != c && d >= 0 && d < n && c >= 0 && c < n) {
                const unsigned long long ki = (unsigned long long)k[i];
                comm[i] = d;
                atomicAdd(&tot[c], 0ull - ki);                 // (two's complement: tot_c -= k_i)
                atomicAdd(&tot[d], ki);
                atomicAdd(&size[c], -1);
                atomicAdd(&size[d], 1);
                one = 1;
            }
        }
    }
    one = lv_wave_sum(one);
    if ((threadIdx.x & 63) == 0 && one) atomicAdd(moved, (unsigned long long)one);
}

__device__ __forceinline__ long long lv_group_sum(long long v) {
#pragma unroll
    for (int s = LV_GROUP / 2; s > 0; s >>= 1) v += __shfl_xor(v, s);       // (every lane of the wave is here)
    return v;
}

__global__ __launch_bounds__(256) void lv_internal_kernel(const long long* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                          const long long* __restrict__ w, long long nnz, long long n,
                                                          const long long* __restrict__ loop, const int32_t* __restrict__ comm,
                                                          unsigned long long* __restrict__ inside) {
    const int l = threadIdx.x & (LV_GROUP - 1);
    const long long row = (long long)blockIdx.x * (256 / LV_GROUP) + threadIdx.x / LV_GROUP;
    long long acc = 0;
    int c = -1;
    if (row < n) {
        c = comm[row];
        long long e0 = rowptr[row], e1 = rowptr[row + 1];
        e0 = e0 < 0 ? 0 : e0;
        e1 = e1 > nnz ? nnz : e1;
        for (long long e = e0 + l; e < e1; e += LV_GROUP) {
            const long long j = col[e];
            if (j >= 0 && j < n && comm[j] == c) acc += w[e];
        }
    }
    acc = lv_group_sum(acc);
    if (row < n && l == 0 && c >= 0 && c < n) atomicAdd(&inside[c], (unsigned long long)(acc + loop[row]));
}

__global__ __launch_bounds__(256) void lv_quantise_kernel(const long long* __restrict__ rowptr, const float* __restrict__ val,
                                                          long long nnz, long long n, long long* __restrict__ w,
                                                          long long* __restrict__ k) {
    const int l = threadIdx.x & (LV_GROUP - 1);
    const long long row = (long long)blockIdx.x * (256 / LV_GROUP) + threadIdx.x / LV_GROUP;
    long long acc = 0;
    if (row < n) {
        long long e0 = rowptr[row], e1 = rowptr[row + 1];
        e0 = e0 < 0 ? 0 : e0;
        e1 = e1 > nnz ? nnz : e1;
        for (long long e = e0 + l; e < e1; e += LV_GROUP) {
            const double x = (double)val[e] * 1048576.0;      // (exact: 24 bits times a power of two)
            long long q = 1;
            if (x >= 4503599627370496.0) q = LV_TWO_M_MAX;    // (the total is then refused)
            else if (x >= 1.0) q = (long long)__builtin_rint(x);      // round half to even
            w[e] = q;
            acc += q;
        }
    }
    acc = lv_group_sum(acc);
    if (row < n && l == 0) k[row] = acc;
}

}  // namespace

extern "C" long long jamie_louvain_workspace(const long long* lens, long long count) {
    if (!lens || count < 1) return 0;
    long long slots = 0;
    for (long long r = 0; r < count; ++r) {
        if (lens[r] < 0 || lens[r] >= LV_NODES_MAX) return 0;
        slots += lv_slots(lens[r]);
    }
    return slots * 12;
}

extern "C" int jamie_louvain_quantise(const long long* rowptr, const float* val, long long nnz, long long n, long long* w,
                                      long long* k, void* stream) {
    JAMIE_ARG(rowptr && k && (nnz == 0 || (val && w)), "null pointer");
    JAMIE_ARG(n >= 1 && n < LV_NODES_MAX && nnz >= 0, "1 <= n < 2^31, nnz >= 0");
    hipLaunchKernelGGL(lv_quantise_kernel, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, (hipStream_t)stream, rowptr, val, nnz, n, w, k);
    return jamie_launch_status("jamie_louvain_quantise");
}

extern "C" int jamie_louvain_move(const long long* rowptr, const int32_t* col, const long long* w, long long nnz, long long n,
                                  const long long* k, const int32_t* comm, const long long* tot, const int32_t* size, double gamma,
                                  long long two_m, const int32_t* nodes, long long n_short, long long n_long, long long n_global,
                                  const long long* slot_off, long long n_slots, void* ws, long long ws_bytes, int32_t* target,
                                  int32_t* flag, void* stream) {
    JAMIE_ARG(rowptr && k && comm && tot && size && nodes && target && flag && (nnz == 0 || (col && w)), "null pointer");
    JAMIE_ARG(n >= 1 && n < LV_NODES_MAX && nnz >= 0, "1 <= n < 2^31, nnz >= 0");
    JAMIE_ARG(two_m >= 1 && two_m < LV_TWO_M_MAX, "1 <= two_m < 2^52");
    JAMIE_ARG(gamma > 0.0 && gamma <= 1.79e308, "gamma must be positive and finite");
    JAMIE_ARG(n_short >= 0 && n_long >= 0 && n_global >= 0 && n_short + n_long + n_global <= n, "the three counts are >= 0 and at most n in all");
    JAMIE_ARG((const void*)target != (const void*)comm, "target must differ from comm");
    JAMIE_ARG(n_global == 0 || (slot_off && ws && n_slots >= 1 && n_slots <= ws_bytes / 12 && ((uintptr_t)ws & 7) == 0),
              "rows beyond the LDS cap need slot_off and an 8-byte aligned workspace of 12 n_slots bytes");
    hipStream_t st = (hipStream_t)stream;
    const LvGraph g = {rowptr, col, w, nnz, n, k, comm, tot, size, gamma, (double)two_m};
    if (n_short)
        hipLaunchKernelGGL(lv_move_short_kernel, dim3((unsigned)((n_short + 3) / 4)), dim3(256), 0, st, g, nodes, n_short, target, flag);
    if (n_long)
        hipLaunchKernelGGL(lv_move_long_kernel, dim3((unsigned)n_long), dim3(256), 0, st, g, nodes + n_short, target, flag);
    if (n_global) {
        unsigned long long* sums = (unsigned long long*)ws;
        int* keys = (int*)(sums + n_slots);
        if (hipMemsetAsync(sums, 0, (size_t)n_slots * 8, st) != hipSuccess || hipMemsetAsync(keys, 0xff, (size_t)n_slots * 4, st) != hipSuccess)
            return jamie_launch_status("jamie_louvain_move");
        hipLaunchKernelGGL(lv_move_global_kernel, dim3((unsigned)n_global), dim3(256), 0, st, g, nodes + n_short + n_long, slot_off,
                           n_slots, sums, keys, target, flag);
    }
    return jamie_launch_status("jamie_louvain_move");
}

extern "C" int jamie_louvain_apply(const int32_t* nodes, long long count, const int32_t* target, const long long* k, int32_t* comm,
                                   long long* tot, int32_t* size, long long* moved, long long n, void* stream) {
    JAMIE_ARG(nodes && target && k && comm && tot && size && moved, "null pointer");
    JAMIE_ARG(n >= 1 && n < LV_NODES_MAX && count >= 1 && count <= n, "1 <= count <= n < 2^31");
    JAMIE_ARG((const void*)target != (const void*)comm, "target must differ from comm");
    hipLaunchKernelGGL(lv_apply_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, (hipStream_t)stream, nodes, count, target, k,
                       comm, (unsigned long long*)tot, size, (unsigned long long*)moved, n);
    return jamie_launch_status("jamie_louvain_apply");
}

extern "C" int jamie_louvain_internal(const long long* rowptr, const int32_t* col, const long long* w, long long nnz, long long n,
                                      const long long* loop, const int32_t* comm, long long* inside, void* stream) {
    JAMIE_ARG(rowptr && loop && comm && inside && (nnz == 0 || (col && w)), "null pointer");
    JAMIE_ARG(n >= 1 && n < LV_NODES_MAX && nnz >= 0, "1 <= n < 2^31, nnz >= 0");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(inside, 0, (size_t)n * 8, st) != hipSuccess) return jamie_launch_status("jamie_louvain_internal");
    hipLaunchKernelGGL(lv_internal_kernel, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, st, rowptr, col, w, nnz, n, loop, comm,
                       (unsigned long long*)inside);
    return jamie_launch_status("jamie_louvain_internal");
}

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
// The bins, the table and the search for the best candidate are csrc/community_rows.h's, shared with csrc/leiden.hip; what is the
// move phase's own is the policy `LvMove` below.  A row's candidates are gathered in an open-addressing table keyed by community id
// with int64 sums (a compare-and-swap claims a slot, an integer add fills it), the node's own community aside in a register.  Every
// sum is an integer sum, so the order of the atomics does not show; the best candidate is taken under the total order (gain
// descending, id ascending), so the order of the slots does not show either.  The gain is formed in fp64 in the one operation order
// of the definition, without contraction.  No floating-point atomics.  Bit-identical from run to run.
#include "community_rows.h"

namespace {

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

// the move phase as the policy of csrc/community_rows.h: the table is keyed by the community of the entry's other end
struct LvMove {
    typedef LvNode Node;
    const LvGraph& g;

    __device__ __forceinline__ bool admit(int, int&) const { return true; }

    // one entry of a row: its weight goes to `own` or into the table
    __device__ __forceinline__ void gather(long long e, int c, int* keys, unsigned long long* sums, unsigned mask, long long& own) const {
        const long long j = g.col[e];
        if (j < 0 || j >= g.n) return;
        const int d = g.comm[j];
        const long long we = g.w[e];
        if (d == c) own += we;
        else if (d >= 0 && d < g.n) cr_table_add(keys, sums, mask, d, (unsigned long long)we);
    }

    __device__ __forceinline__ LvNode node(int i, int c, long long own) const {
#pragma clang fp contract(off)
        LvNode nd;
        const long long ki = g.k[i];
        nd.c = c;
        nd.single = g.size[c] == 1;
        nd.gki = g.gamma * (double)ki;
        nd.gain_c = lv_gain(own, nd.gki, g.tot[c] - ki, g.two_m);
        return nd;
    }

    __device__ __forceinline__ bool scans(const LvNode&) const { return true; }

    __device__ __forceinline__ void offer(const LvNode& nd, int d, long long kid, CrBest& best) const {
        if (nd.single && d > nd.c && g.size[d] == 1) return;      // the singleton rule
        const double gain = lv_gain(kid, nd.gki, g.tot[d], g.two_m);
        if (gain > nd.gain_c && cr_better(gain, d, best)) {
            best.gain = gain;
            best.id = d;
        }
    }

    __device__ __forceinline__ int stay(int, int c) const { return c; }
};

__global__ __launch_bounds__(256) void lv_move_short_kernel(LvGraph g, const int32_t* __restrict__ nodes, long long count,
                                                            int32_t* __restrict__ target, int32_t* __restrict__ flag) {
    __shared__ int keys[4][CR_SHORT_SLOTS];
    __shared__ unsigned long long sums[4][CR_SHORT_SLOTS];
    cr_short_rows(LvMove{g}, nodes, count, keys[threadIdx.x >> 6], sums[threadIdx.x >> 6], target, flag);
}

__global__ __launch_bounds__(256) void lv_move_long_kernel(LvGraph g, const int32_t* __restrict__ nodes, int32_t* __restrict__ target,
                                                           int32_t* __restrict__ flag) {
    __shared__ int keys[CR_LONG_SLOTS];
    __shared__ unsigned long long sums[CR_LONG_SLOTS];
    cr_long_row(LvMove{g}, nodes, keys, sums, target, flag);
}

__global__ __launch_bounds__(256) void lv_move_global_kernel(LvGraph g, const int32_t* __restrict__ nodes,
                                                             const long long* __restrict__ slot_off, long long n_slots,
                                                             unsigned long long* sums, int* keys, int32_t* __restrict__ target,
                                                             int32_t* __restrict__ flag) {
    cr_global_row(LvMove{g}, nodes, slot_off, n_slots, sums, keys, target, flag);
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
    one = cr_wave_sum(one);
    if ((threadIdx.x & 63) == 0 && one) atomicAdd(moved, (unsigned long long)one);
}

__global__ __launch_bounds__(256) void lv_internal_kernel(const long long* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                          const long long* __restrict__ w, long long nnz, long long n,
                                                          const long long* __restrict__ loop, const int32_t* __restrict__ comm,
                                                          unsigned long long* __restrict__ inside) {
    const long long row = cr_group_row();
    const int c = row < n ? comm[row] : -1;
    const long long acc = cr_group_row_sum(rowptr, nnz, n, row, [&](long long e) -> long long {
        const long long j = col[e];
        if (j >= 0 && j < n && comm[j] == c) return w[e];
        return 0;
    });
    if (row < n && (threadIdx.x & (CR_GROUP - 1)) == 0 && c >= 0 && c < n) atomicAdd(&inside[c], (unsigned long long)(acc + loop[row]));
}

__global__ __launch_bounds__(256) void lv_quantise_kernel(const long long* __restrict__ rowptr, const float* __restrict__ val,
                                                          long long nnz, long long n, long long* __restrict__ w,
                                                          long long* __restrict__ k) {
    const long long row = cr_group_row();
    const long long acc = cr_group_row_sum(rowptr, nnz, n, row, [&](long long e) -> long long {
        const double x = (double)val[e] * 1048576.0;          // (exact: 24 bits times a power of two)
        long long q = 1;
        if (x >= 4503599627370496.0) q = CR_TWO_M_MAX;        // (the total is then refused)
        else if (x >= 1.0) q = (long long)__builtin_rint(x);  // round half to even
        w[e] = q;
        return q;
    });
    if (row < n && (threadIdx.x & (CR_GROUP - 1)) == 0) k[row] = acc;
}

}  // namespace

extern "C" long long jamie_louvain_workspace(const long long* lens, long long count) {
    if (!lens || count < 1) return 0;
    long long slots = 0;
    for (long long r = 0; r < count; ++r) {
        if (lens[r] < 0 || lens[r] >= CR_NODES_MAX) return 0;
        slots += cr_slots(lens[r]);
    }
    return slots * 12;
}

extern "C" int jamie_louvain_quantise(const long long* rowptr, const float* val, long long nnz, long long n, long long* w,
                                      long long* k, void* stream) {
    JAMIE_ARG(rowptr && k && (nnz == 0 || (val && w)), "null pointer");
    JAMIE_ARG(n >= 1 && n < CR_NODES_MAX && nnz >= 0, "1 <= n < 2^31, nnz >= 0");
    hipLaunchKernelGGL(lv_quantise_kernel, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, (hipStream_t)stream, rowptr, val, nnz, n, w, k);
    return jamie_launch_status("jamie_louvain_quantise");
}

extern "C" int jamie_louvain_move(const long long* rowptr, const int32_t* col, const long long* w, long long nnz, long long n,
                                  const long long* k, const int32_t* comm, const long long* tot, const int32_t* size, double gamma,
                                  long long two_m, const int32_t* nodes, long long n_short, long long n_long, long long n_global,
                                  const long long* slot_off, long long n_slots, void* ws, long long ws_bytes, int32_t* target,
                                  int32_t* flag, void* stream) {
    JAMIE_ARG(rowptr && k && comm && tot && size && nodes && target && flag && (nnz == 0 || (col && w)), "null pointer");
    JAMIE_ARG((const void*)target != (const void*)comm, "target must differ from comm");
    const LvGraph g = {rowptr, col, w, nnz, n, k, comm, tot, size, gamma, (double)two_m};
    return cr_launch(__func__, g, two_m, nodes, n_short, n_long, n_global, slot_off, n_slots, ws, ws_bytes, target, flag,
                     (hipStream_t)stream, lv_move_short_kernel, lv_move_long_kernel, lv_move_global_kernel);
}

extern "C" int jamie_louvain_apply(const int32_t* nodes, long long count, const int32_t* target, const long long* k, int32_t* comm,
                                   long long* tot, int32_t* size, long long* moved, long long n, void* stream) {
    JAMIE_ARG(nodes && target && k && comm && tot && size && moved, "null pointer");
    JAMIE_ARG(n >= 1 && n < CR_NODES_MAX && count >= 1 && count <= n, "1 <= count <= n < 2^31");
    JAMIE_ARG((const void*)target != (const void*)comm, "target must differ from comm");
    hipLaunchKernelGGL(lv_apply_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, (hipStream_t)stream, nodes, count, target, k,
                       comm, (unsigned long long*)tot, size, (unsigned long long*)moved, n);
    return jamie_launch_status("jamie_louvain_apply");
}

extern "C" int jamie_louvain_internal(const long long* rowptr, const int32_t* col, const long long* w, long long nnz, long long n,
                                      const long long* loop, const int32_t* comm, long long* inside, void* stream) {
    JAMIE_ARG(rowptr && loop && comm && inside && (nnz == 0 || (col && w)), "null pointer");
    JAMIE_ARG(n >= 1 && n < CR_NODES_MAX && nnz >= 0, "1 <= n < 2^31, nnz >= 0");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(inside, 0, (size_t)n * 8, st) != hipSuccess) return jamie_launch_status("jamie_louvain_internal");
    hipLaunchKernelGGL(lv_internal_kernel, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, st, rowptr, col, w, nnz, n, loop, comm,
                       (unsigned long long*)inside);
    return jamie_launch_status("jamie_louvain_internal");
}

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
// The bins, the node lists, the workspace, the open-addressing table (a compare-and-swap claims a slot, an integer add fills it) and
// the search for the best candidate are csrc/community_rows.h's, shared with csrc/louvain.hip; what is the refinement's own is the
// policy `LdRefine` below: the table is keyed by the sub-community ref[j] and filled only from the entries inside the node's
// community.  Every sum is an integer sum, the two conditions and the gain are formed in fp64 in the one operation order of the
// definition, without contraction, and the best candidate is taken under the total order (gain descending, id ascending).  No
// floating-point atomics.  Bit-identical from run to run.
#include "community_rows.h"

namespace {

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

// what a node needs beside its row
struct LdNode {
    int i;
    long long inside, T;
    double gki;
};

// the refinement as the policy of csrc/community_rows.h
struct LdRefine {
    typedef LdNode Node;
    const LdGraph& g;

    // a node that is no longer alone has nothing to gather: it stays in its part
    __device__ __forceinline__ bool admit(int i, int& leave) const {
        if (ld_alone(g, i)) return true;
        leave = g.ref[i];
        return false;
    }

    // one entry of a row: inside the community c its weight goes to `inside` and into the table under its sub-community
    __device__ __forceinline__ void gather(long long e, int c, int* keys, unsigned long long* sums, unsigned mask, long long& inside) const {
        const long long j = g.col[e];
        if (j < 0 || j >= g.n || g.comm[j] != c) return;
        const long long we = g.w[e];
        const int s = g.ref[j];
        inside += we;
        if (s >= 0 && s < g.n) cr_table_add(keys, sums, mask, s, (unsigned long long)we);
    }

    __device__ __forceinline__ LdNode node(int i, int c, long long inside) const {
#pragma clang fp contract(off)
        LdNode nd;
        nd.i = i;
        nd.inside = inside;
        nd.T = g.tot[c];
        nd.gki = g.gamma * (double)g.k[i];
        return nd;
    }

    // only a node well connected to its community looks for a part to join
    __device__ __forceinline__ bool scans(const LdNode& nd) const { return ld_well(g, nd.inside, g.k[nd.i], nd.T); }

    __device__ __forceinline__ void offer(const LdNode& nd, int s, long long kis, CrBest& best) const {
#pragma clang fp contract(off)
        if (s == nd.i) return;                                               // (an alone node has no entry of its own)
        const long long rt = g.rtot[s];
        if (s > nd.i && g.rsize[s] == 1) return;                             // the singleton rule
        if (!ld_well(g, g.cut[s], rt, nd.T)) return;
        const double gain = (double)kis - (nd.gki * (double)rt) / g.two_m;
        if (gain > 0.0 && cr_better(gain, s, best)) {
            best.gain = gain;
            best.id = s;
        }
    }

    __device__ __forceinline__ int stay(int i, int) const { return i; }
};

__global__ __launch_bounds__(256) void ld_refine_short_kernel(LdGraph g, const int32_t* __restrict__ nodes, long long count,
                                                              int32_t* __restrict__ target, int32_t* __restrict__ flag) {
    __shared__ int keys[4][CR_SHORT_SLOTS];
    __shared__ unsigned long long sums[4][CR_SHORT_SLOTS];
    cr_short_rows(LdRefine{g}, nodes, count, keys[threadIdx.x >> 6], sums[threadIdx.x >> 6], target, flag);
}

__global__ __launch_bounds__(256) void ld_refine_long_kernel(LdGraph g, const int32_t* __restrict__ nodes, int32_t* __restrict__ target,
                                                             int32_t* __restrict__ flag) {
    __shared__ int keys[CR_LONG_SLOTS];
    __shared__ unsigned long long sums[CR_LONG_SLOTS];
    cr_long_row(LdRefine{g}, nodes, keys, sums, target, flag);
}

__global__ __launch_bounds__(256) void ld_refine_global_kernel(LdGraph g, const int32_t* __restrict__ nodes,
                                                               const long long* __restrict__ slot_off, long long n_slots,
                                                               unsigned long long* sums, int* keys, int32_t* __restrict__ target,
                                                               int32_t* __restrict__ flag) {
    cr_global_row(LdRefine{g}, nodes, slot_off, n_slots, sums, keys, target, flag);
}

__global__ __launch_bounds__(256) void ld_cut_kernel(const long long* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                     const long long* __restrict__ w, long long nnz, long long n,
                                                     const int32_t* __restrict__ comm, const int32_t* __restrict__ ref,
                                                     unsigned long long* __restrict__ cut) {
    const long long row = cr_group_row();
    const int c = row < n ? comm[row] : -1, s = row < n ? ref[row] : -1;
    const long long acc = cr_group_row_sum(rowptr, nnz, n, row, [&](long long e) -> long long {
        const long long j = col[e];
        if (j >= 0 && j < n && comm[j] == c && ref[j] != s) return w[e];
        return 0;
    });
    if (row < n && (threadIdx.x & (CR_GROUP - 1)) == 0 && acc != 0 && s >= 0 && s < n) atomicAdd(&cut[s], (unsigned long long)acc);
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
    merged = cr_wave_sum(merged);
    cancelled = cr_wave_sum(cancelled);
    if ((threadIdx.x & 63) == 0) {
        if (merged) atomicAdd(&counts[0], (unsigned long long)merged);
        if (cancelled) atomicAdd(&counts[1], (unsigned long long)cancelled);
    }
}

}  // namespace

extern "C" int jamie_leiden_cut(const long long* rowptr, const int32_t* col, const long long* w, long long nnz, long long n,
                                const int32_t* comm, const int32_t* ref, long long* cut, void* stream) {
    JAMIE_ARG(rowptr && comm && ref && cut && (nnz == 0 || (col && w)), "null pointer");
    JAMIE_ARG(n >= 1 && n < CR_NODES_MAX && nnz >= 0, "1 <= n < 2^31, nnz >= 0");
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
    JAMIE_ARG((const void*)target != (const void*)ref && (const void*)target != (const void*)comm, "target must differ from ref and comm");
    const LdGraph g = {rowptr, col, w, nnz, n, k, comm, tot, ref, rtot, rsize, cut, gamma, (double)two_m};
    return cr_launch(__func__, g, two_m, nodes, n_short, n_long, n_global, slot_off, n_slots, ws, ws_bytes, target, flag,
                     (hipStream_t)stream, ld_refine_short_kernel, ld_refine_long_kernel, ld_refine_global_kernel);
}

extern "C" int jamie_leiden_apply(const int32_t* nodes, long long count, const int32_t* target, const long long* k, int32_t* ref,
                                  long long* rtot, int32_t* rsize, long long* counts, long long n, void* stream) {
    JAMIE_ARG(nodes && target && k && ref && rtot && rsize && counts, "null pointer");
    JAMIE_ARG(n >= 1 && n < CR_NODES_MAX && count >= 1 && count <= n, "1 <= count <= n < 2^31");
    JAMIE_ARG((const void*)target != (const void*)ref, "target must differ from ref");
    hipLaunchKernelGGL(ld_apply_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, (hipStream_t)stream, nodes, count, target, k,
                       ref, (unsigned long long*)rtot, rsize, (unsigned long long*)counts, n);
    return jamie_launch_status("jamie_leiden_apply");
}

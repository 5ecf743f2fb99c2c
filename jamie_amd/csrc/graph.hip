// Graph structure on the device (include/jamie_hip.h "Graph structure on the device"; jamie_amd/graph.py): connected components of
// a CSR graph by synchronous min-label hooking, and the kBET statistic of every cell from its neighbour lists.  DESIGN.md §26.
//
//   gr_hook_kernel   16 lanes per row, 16 rows per workgroup; a row of more than 256 entries is then taken by the whole workgroup
//   gr_jump_kernel   a thread per node: out[i] = in[in[i]]
//   kb_stat_kernel   16 lanes per cell, 16 cells per workgroup: the counts in LDS, the sum by one lane in ascending category
//
// A hook launch reads `root` (the round's input) and writes `parent` by integer atomicMin alone, so the array it leaves is a
// function of its input, whatever the order of the atomics.  With a = root[i]: the entries with root[j] > a hook root[j] under a,
// one atomic each; the entries with root[j] < a all aim at parent[a], so the row takes their minimum across its lanes and hooks a
// under it with one atomic -- integer min is associative, the array is the one the per-entry form leaves.  No kernel waits for
// another thread's store.  The kBET sum is formed in fp64 in the one operation order of the definition, without contraction.  No
// floating-point atomics.  Bit-identical from run to run.
#include "common.h"

namespace {

constexpr int GR_GROUP = 16;                  // lanes per row of the hook
constexpr int GR_ROWS = 256 / GR_GROUP;       // rows per workgroup
constexpr int GR_LONG = 256;                  // entries of a row beyond which the workgroup takes it
constexpr long long GR_NODES_MAX = 1ll << 31;
constexpr int GR_NONE = 0x7fffffff;
constexpr int KB_KMAX = 128;
constexpr int KB_BMAX = 64;
constexpr int KB_GROUP = 16;                  // lanes per cell
constexpr int KB_CELLS = 256 / KB_GROUP;      // cells per workgroup

struct GrGraph {
    const long long* rowptr;
    const int32_t* col;
    long long nnz, n;
    const int32_t* group;
    const int32_t* root;
};

// raises *flag; the load keeps all but the first few of a launch from storing to the one address
__device__ __forceinline__ void gr_raise(int32_t* flag) {
    if (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0)
        __hip_atomic_store(flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the extent of row i clamped to the arrays, its root (-1: not a node id, the row hooks nothing) and its group
__device__ __forceinline__ void gr_row(const GrGraph& g, long long i, long long& e0, long long& e1, int& a, int& gi) {
    e0 = g.rowptr[i];
    e1 = g.rowptr[i + 1];
    e0 = e0 < 0 ? 0 : e0;
    e1 = e1 > g.nnz ? g.nnz : e1;
    if (e1 < e0) e1 = e0;
    a = g.root[i];
    if (a < 0 || a >= g.n) a = -1;
    gi = g.group ? g.group[i] : 0;
}

// entry e of row i (root a, group gi): a larger root is hooked under a here, a smaller one goes into the row's minimum m
__device__ __forceinline__ void gr_entry(const GrGraph& g, long long e, long long i, int a, int gi, int32_t* __restrict__ parent, int& m,
                                         bool& any) {
    const long long j = g.col[e];
    if (j < 0 || j >= g.n || j == i) return;
    if (g.group && g.group[j] != gi) return;
    const int b = g.root[j];
    if (b == a || b < 0 || b >= g.n) return;
    any = true;
    if (b > a) atomicMin(&parent[b], a);
    else m = b < m ? b : m;
}

__global__ __launch_bounds__(256) void gr_hook_kernel(GrGraph g, int32_t* __restrict__ parent, int32_t* __restrict__ changed) {
    __shared__ int row_min[GR_ROWS];
    __shared__ int is_long[GR_ROWS];
    const int l = threadIdx.x & (GR_GROUP - 1), r = threadIdx.x / GR_GROUP;
    const long long first = (long long)blockIdx.x * GR_ROWS, row = first + r;
    long long e0 = 0, e1 = 0;
    int a = -1, gi = 0, m = GR_NONE;
    bool any = false;
    if (row < g.n) gr_row(g, row, e0, e1, a, gi);
    const bool lng = e1 - e0 > GR_LONG;
    if (a >= 0 && !lng)
        for (long long e = e0 + l; e < e1; e += GR_GROUP) gr_entry(g, e, row, a, gi, parent, m, any);
#pragma unroll
    for (int s = GR_GROUP / 2; s > 0; s >>= 1) {              // (every lane of the wave is here)
        const int o = __shfl_xor(m, s);
        m = o < m ? o : m;
    }
    if (l == 0) {
        if (m < a) atomicMin(&parent[a], m);
        is_long[r] = lng && a >= 0;
        row_min[r] = GR_NONE;
    }
    if (__syncthreads_or(lng && a >= 0)) {                    // (the same in every thread of the workgroup)
        for (int q = 0; q < GR_ROWS; ++q) {
            if (!is_long[q]) continue;
            const long long i = first + q;
            gr_row(g, i, e0, e1, a, gi);
            m = GR_NONE;
            for (long long e = e0 + threadIdx.x; e < e1; e += 256) gr_entry(g, e, i, a, gi, parent, m, any);
#pragma unroll
            for (int s = 32; s > 0; s >>= 1) {
                const int o = __shfl_xor(m, s);
                m = o < m ? o : m;
            }
            if ((threadIdx.x & 63) == 0 && m != GR_NONE) atomicMin(&row_min[q], m);
            __syncthreads();
            if (threadIdx.x == 0 && row_min[q] < a) atomicMin(&parent[a], row_min[q]);
        }
    }
    if (__syncthreads_or(any) && threadIdx.x == 0) gr_raise(changed);
}

__global__ __launch_bounds__(256) void gr_jump_kernel(const int32_t* __restrict__ in, int32_t* __restrict__ out, long long n,
                                                      int32_t* __restrict__ changed) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    bool any = false;
    if (i < n) {
        const int v = in[i];
        const int u = v >= 0 && v < n ? in[v] : v;            // (a value that is no node id stays)
        out[i] = u;
        any = u != v;
    }
    if (__syncthreads_or(any) && threadIdx.x == 0) gr_raise(changed);
}

__global__ __launch_bounds__(256) void kb_stat_kernel(const int32_t* __restrict__ idx, long long N, int K, const int32_t* __restrict__ codes,
                                                      int B, const double* __restrict__ expected, int n_e,
                                                      const int32_t* __restrict__ erow, double* __restrict__ stat,
                                                      int32_t* __restrict__ df, int32_t* __restrict__ counts) {
#pragma clang fp contract(off)
    __shared__ int cnt[KB_CELLS][KB_BMAX];
    __shared__ double term[KB_CELLS][KB_BMAX];                // (o_b - e_b)^2 / e_b; -1: expected is 0
    __shared__ int total[KB_CELLS], unexpected[KB_CELLS];
    const int l = threadIdx.x & (KB_GROUP - 1), c = threadIdx.x / KB_GROUP;
    const long long i = (long long)blockIdx.x * KB_CELLS + c;
    for (int b = l; b < B; b += KB_GROUP) cnt[c][b] = 0;
    if (l == 0) total[c] = unexpected[c] = 0;
    __syncthreads();
    if (i < N)
        for (int t = l; t < K; t += KB_GROUP) {
            const long long j = idx[i * K + t];
            if (j < 0 || j >= N) continue;
            const int b = codes[j];
            if (b < 0 || b >= B) continue;
            atomicAdd(&cnt[c][b], 1);
            atomicAdd(&total[c], 1);
        }
    __syncthreads();
    int er = 0;
    if (i < N) {
        er = erow ? erow[i] : 0;
        const bool have = er >= 0 && er < n_e;                // (a cell without a row of `expected` is not tested)
        const double k = (double)total[c];
        for (int b = l; b < B; b += KB_GROUP) {
            const int o = cnt[c][b];
            if (counts) counts[i * B + b] = o;
            const double f = have ? expected[(long long)er * B + b] : 0.0;
            if (f > 0.0) {
                const double e = k * f;
                const double d = (double)o - e;
                term[c][b] = (d * d) / e;
            } else {
                term[c][b] = -1.0;
                if (o > 0 || !have) atomicOr(&unexpected[c], 1);
            }
        }
    }
    __syncthreads();
    if (i < N && l == 0) {
        double s = 0.0;
        int cats = 0;
        for (int b = 0; b < B; ++b) {
            const double t = term[c][b];
            if (t >= 0.0) {
                s += t;
                ++cats;
            }
        }
        const bool tested = total[c] > 0 && cats >= 2 && !unexpected[c];
        stat[i] = tested ? s : __builtin_nan("");
        df[i] = tested ? cats - 1 : 0;
    }
}

}  // namespace

extern "C" int jamie_graph_hook(const long long* rowptr, const int32_t* col, long long nnz, long long n, const int32_t* group,
                                const int32_t* root, int32_t* parent, int32_t* changed, void* stream) {
    JAMIE_ARG(rowptr && root && parent && changed && (nnz == 0 || col), "null pointer");
    JAMIE_ARG(n >= 1 && n < GR_NODES_MAX && nnz >= 0, "1 <= n < 2^31, nnz >= 0");
    JAMIE_ARG((const void*)parent != (const void*)root, "parent must differ from root");
    const GrGraph g = {rowptr, col, nnz, n, group, root};
    hipLaunchKernelGGL(gr_hook_kernel, dim3((unsigned)((n + GR_ROWS - 1) / GR_ROWS)), dim3(256), 0, (hipStream_t)stream, g, parent, changed);
    return jamie_launch_status("jamie_graph_hook");
}

extern "C" int jamie_graph_jump(const int32_t* in, int32_t* out, long long n, int32_t* changed, void* stream) {
    JAMIE_ARG(in && out && changed, "null pointer");
    JAMIE_ARG(n >= 1 && n < GR_NODES_MAX, "1 <= n < 2^31");
    JAMIE_ARG((const void*)in != (const void*)out, "out must differ from in");
    hipLaunchKernelGGL(gr_jump_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, in, out, n, changed);
    return jamie_launch_status("jamie_graph_jump");
}

extern "C" int jamie_kbet_stat(const int32_t* idx, long long N, int K, const int32_t* codes, int B, const double* expected, int n_e,
                               const int32_t* erow, double* stat, int32_t* df, int32_t* counts, void* stream) {
    JAMIE_ARG(idx && codes && expected && stat && df, "null pointer");
    JAMIE_ARG(N >= 1 && N < GR_NODES_MAX && K >= 1 && K <= KB_KMAX, "1 <= N < 2^31, 1 <= K <= 128");
    JAMIE_ARG(B >= 1 && B <= KB_BMAX && n_e >= 1, "1 <= B <= 64, n_e >= 1");
    hipLaunchKernelGGL(kb_stat_kernel, dim3((unsigned)((N + KB_CELLS - 1) / KB_CELLS)), dim3(256), 0, (hipStream_t)stream, idx, N, K, codes,
                       B, expected, n_e, erow, stat, df, counts);
    return jamie_launch_status("jamie_kbet_stat");
}

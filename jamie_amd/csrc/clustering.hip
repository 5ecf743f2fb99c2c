// Clustering on the device (include/jamie_hip.h "Clustering on the device"; jamie_amd/clustering.py): Lloyd's k-means of one
// [N, L] fp32 matrix, k <= 1024, with assignment and cluster sums in ONE pass over the rows; the running-minimum and weighted-pick
// kernels of k-means++ seeding; the contingency table of two code arrays.  Nothing of size N x k is stored.
//
// The step is the row tile of the cross search (pair_tile.h `pair_tile`, 128 rows x 128 centres, q by the chain of `q_step`) with a
// running (q, j) minimum per row in registers in place of the lists.  A workgroup owns a contiguous segment of rows.  After the
// centre tiles of a row tile its 128 labels go to LDS and the rows are added into an fp64 table [k, L]: thread (feature c, group
// g) owns the clusters j with j % groups == g and walks the 128 rows in ascending order, so every element of the table has ONE
// owner and one order of additions: no floating-point atomics.  The table lives in LDS while k L <= TAB_MAX (3072 elements, 24 KB
// beside the 33 KB of staged operands: two workgroups per CU), else in the workgroup's slab of the workspace (the same owner, plain
// loads and stores).  A reduce kernel adds the segments' tables in segment order, forms the new centres and the shift, and a
// one-workgroup kernel adds the scalars, counts the iteration and raises `done` when a stop rule holds: launches that find `done`
// raised return at once, so the host enqueues iterations in batches without reading anything back in between.
#include "pair_tile.h"

namespace {

constexpr int KM_KMAX = 1024;     // clusters
constexpr int TAB_MAX = 3072;     // elements of the fp64 table kept in LDS
constexpr int PICK_BLOCK = 1024;  // elements per block total of the weighted pick

__device__ __forceinline__ double wave_sum_f64(double v) {   // (a + b and b + a are the same bits: every lane ends with the same sum)
    v += __shfl_xor(v, 32);
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 8);
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 1);
    return v;
}

// state[0] = done, state[1] = iterations completed, state[2] = a rule other than max_iter stopped it
template <bool LDS_TAB>
__global__ __launch_bounds__(256, 2) void kmeans_step_kernel(const float* __restrict__ X, long long N, int L, int vec,
                                                             const float* __restrict__ C, int k, int32_t* __restrict__ labels,
                                                             float* __restrict__ minq, long long seg_len,
                                                             double* __restrict__ slab, double* __restrict__ seg_inertia,
                                                             int* __restrict__ cnt_slab, int* __restrict__ seg_changed,
                                                             const int32_t* __restrict__ state) {
    if (state[0]) return;                                  // (the same answer in every thread of every workgroup)
    __shared__ __attribute__((aligned(16))) float smem[KC * (128 + 4) + KC * LDJ];
    __shared__ int2 lab_s[128];                            // (label, owner group) of the tile's rows; label -1: no such row
    __shared__ float mq_s[128];
    __shared__ int cnt_s[KM_KMAX];
    __shared__ double tab_s[LDS_TAB ? TAB_MAX : 1];
    __shared__ int chg_s;
    float* Xs = smem;
    float* Ys = smem + KC * (128 + 4);
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const long long r0 = (long long)blockIdx.x * seg_len;
    const long long r1 = r0 + seg_len < N ? r0 + seg_len : N;
    const long long kl = (long long)k * L;
    double* const mine = slab + (long long)blockIdx.x * kl;                    // this segment's table in the workspace
    // the owner rule: `groups` groups of L threads (one group of 256 for L >= 256, which then strides over the features)
    const int groups = L >= 256 ? 1 : 256 / L;
    const int cstep = L >= 256 ? 256 : L;
    const int g = L >= 256 ? 0 : tid / L, c_first = L >= 256 ? tid : tid % L;
    const bool owner = g < groups;
    for (int j = tid; j < k; j += 256) cnt_s[j] = 0;
    if (tid == 0) chg_s = 0;
    if constexpr (LDS_TAB) {
        for (int e = tid; e < (int)kl; e += 256) tab_s[e] = 0.0;
    } else if (owner) {                                    // (every element is zeroed by the thread that adds into it)
        for (int j = g; j < k; j += groups)
            for (int c = c_first; c < L; c += cstep) mine[(long long)j * L + c] = 0.0;
    }
    double inertia = 0.0;                                  // (kept by wave 0)
    int changed = 0;
    for (long long i0 = r0; i0 < r1; i0 += 128) {
        float bq[8];
        int bj[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            bq[r] = __builtin_inff();
            bj[r] = 0x7fffffff;
        }
        for (int j0 = 0; j0 < k; j0 += TJ) {
            float acc[8][8];
            pair_tile<2>(X, r1, i0, C, k, j0, L, vec != 0, Xs, Ys, acc);
#pragma unroll
            for (int r = 0; r < 8; ++r)
#pragma unroll
                for (int s = 0; s < 8; ++s) {
                    const int gj = j0 + (s >> 2) * 64 + tx * 4 + (s & 3);
                    float q = acc[r][s];
                    q = q == q ? q : __builtin_inff();     // (inf - inf of huge finite inputs)
                    if (gj < k && key_less(q, gj, bq[r], bj[r])) {
                        bq[r] = q;
                        bj[r] = gj;
                    }
                }
        }
        // the 16 threads of one ty hold the candidates of the same 8 rows: (q, j) is a total order, any tree gives its minimum
#pragma unroll
        for (int r = 0; r < 8; ++r)
#pragma unroll
            for (int m = 1; m < 16; m <<= 1) {
                const float oq = __shfl_xor(bq[r], m);
                const int oj = __shfl_xor(bj[r], m);
                if (key_less(oq, oj, bq[r], bj[r])) {
                    bq[r] = oq;
                    bj[r] = oj;
                }
            }
        if (tx == 0) {
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int row = (r >> 2) * 64 + ty * 4 + (r & 3);
                const bool have = i0 + row < r1;
                lab_s[row] = have ? make_int2(bj[r], bj[r] % groups) : make_int2(-1, -1);
                mq_s[row] = have ? bq[r] : 0.f;
            }
        }
        __syncthreads();
        if (tid < 128 && i0 + tid < r1) {
            const int lab = lab_s[tid].x;
            changed += labels[i0 + tid] != lab;
            labels[i0 + tid] = lab;
            if (minq) minq[i0 + tid] = mq_s[tid];
        }
        if (tid < 64) inertia += wave_sum_f64((double)mq_s[tid] + (double)mq_s[tid + 64]);
        if (owner) {
            const int rows = r1 - i0 < 128 ? (int)(r1 - i0) : 128;
            for (int row = 0; row < rows; ++row) {
                const int2 lo = lab_s[row];
                if (lo.y != g) continue;
                const float* x = X + (i0 + row) * L;
                if constexpr (LDS_TAB) {
                    double* t = tab_s + lo.x * L;
                    for (int c = c_first; c < L; c += cstep) t[c] += (double)x[c];
                } else {
                    double* t = mine + (long long)lo.x * L;
                    for (int c = c_first; c < L; c += cstep) t[c] += (double)x[c];
                }
                if (c_first == 0) cnt_s[lo.x] += 1;
            }
        }
        // (the next tile writes lab_s / mq_s only behind the barriers of its pair tiles, which every thread reaches after this)
    }
    if (changed) atomicAdd(&chg_s, changed);
    __syncthreads();
    if constexpr (LDS_TAB) {
        for (int e = tid; e < (int)kl; e += 256) mine[e] = tab_s[e];
    }
    for (int j = tid; j < k; j += 256) cnt_slab[(long long)blockIdx.x * k + j] = cnt_s[j];
    if (tid == 0) {
        seg_inertia[blockIdx.x] = inertia;
        seg_changed[blockIdx.x] = chg_s;
    }
}

// element (j, c): the segments' sums and counts added in segment order, the new centre, the element's share of the shift
__global__ __launch_bounds__(256) void kmeans_reduce_kernel(const double* __restrict__ slab, const int* __restrict__ cnt_slab,
                                                            long long S, int k, int L, float* __restrict__ C, int update,
                                                            double* __restrict__ sums, long long* __restrict__ counts,
                                                            double* __restrict__ shift_part, const int32_t* __restrict__ state) {
    if (state[0]) return;
    __shared__ double red[4];
    const long long kl = (long long)k * L, e = (long long)blockIdx.x * 256 + threadIdx.x;
    double d2 = 0.0;
    if (e < kl) {
        const int j = (int)(e / L);
        double sum = 0.0;
        long long cnt = 0;
        for (long long s = 0; s < S; ++s) {
            sum += slab[s * kl + e];
            cnt += cnt_slab[s * k + j];
        }
        const float old = C[e];
        const float now = cnt > 0 ? (float)(sum / (double)cnt) : old;      // an empty cluster keeps its centre
        if (update) C[e] = now;
        if (sums) sums[e] = sum;
        if (e % L == 0) counts[j] = cnt;
        const double d = (double)now - (double)old;
        d2 = d * d;
    }
    d2 = wave_sum_f64(d2);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = d2;
    __syncthreads();
    if (threadIdx.x == 0) shift_part[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// the scalars of the iteration in segment (block) order, the iteration count and the stop rules
__global__ __launch_bounds__(256) void kmeans_finish_kernel(const double* __restrict__ seg_inertia, const int* __restrict__ seg_changed,
                                                            long long S, const double* __restrict__ shift_part, int n_parts,
                                                            const long long* __restrict__ counts, int k, double tol_abs,
                                                            int max_iter, double* __restrict__ stats, int32_t* __restrict__ state) {
    if (state[0]) return;
    __shared__ unsigned long long n_changed;
    __shared__ int n_empty;
    if (threadIdx.x == 0) {
        n_changed = 0;
        n_empty = 0;
    }
    __syncthreads();
    unsigned long long ch = 0;
    int empty = 0;
    for (long long s = threadIdx.x; s < S; s += 256) ch += (unsigned long long)seg_changed[s];
    for (int j = threadIdx.x; j < k; j += 256) empty += counts[j] == 0;
    if (ch) atomicAdd(&n_changed, ch);
    if (empty) atomicAdd(&n_empty, empty);
    __syncthreads();
    if (threadIdx.x == 0) {
        double inertia = 0.0, shift = 0.0;
        for (long long s = 0; s < S; ++s) inertia += seg_inertia[s];
        for (int b = 0; b < n_parts; ++b) shift += shift_part[b];
        const int t = state[1] + 1;
        stats[0] = inertia;
        stats[1] = shift;
        stats[2] = (double)n_changed;
        stats[3] = (double)n_empty;
        state[1] = t;
        if ((t >= 2 && n_changed == 0) || shift <= tol_abs) {
            state[2] = 1;
            state[0] = 1;
        } else if (t >= max_iter) {
            state[0] = 1;
        }
    }
}

// minq[i] = q(X[i], X[*row]) (first) or the smaller of that and minq[i]; block 0 copies the centre out.  A row outside [0, N)
// leaves everything as it is.
__global__ __launch_bounds__(256) void kmeans_min_update_kernel(const float* __restrict__ X, long long N, int L,
                                                                const long long* __restrict__ row, float* __restrict__ centre,
                                                                float* __restrict__ minq, int first) {
    const long long cr = *row;
    if (cr < 0 || cr >= N) return;
    const float* cen = X + cr * L;
    if (centre && blockIdx.x == 0)
        for (int c = threadIdx.x; c < L; c += 256) centre[c] = cen[c];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const float* x = X + i * L;
    float q = 0.f;
    for (int c = 0; c < L; ++c) q = q_step(q, x[c], cen[c]);
    q = q == q ? q : __builtin_inff();
    minq[i] = first ? q : (q < minq[i] ? q : minq[i]);
}

// total of block b of 1024 weights in fp64 by the tree v[i] += v[i + stride], stride = 512, 256, ..., 1 (elements past N are 0)
__global__ __launch_bounds__(256) void pick_totals_kernel(const float* __restrict__ w, long long N, double* __restrict__ totals) {
    __shared__ double v[256];
    const long long base = (long long)blockIdx.x * PICK_BLOCK;
    const int t = threadIdx.x;
    double x[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) x[m] = base + t + m * 256 < N ? (double)w[base + t + m * 256] : 0.0;
    v[t] = (x[0] + x[2]) + (x[1] + x[3]);                  // strides 512, then 256
    __syncthreads();
    if (t < 128) v[t] += v[t + 128];
    __syncthreads();
    if (t < 64) {
        double s = v[t] + v[t + 64];
        s += __shfl_down(s, 32);
        s += __shfl_down(s, 16);
        s += __shfl_down(s, 8);
        s += __shfl_down(s, 4);
        s += __shfl_down(s, 2);
        s += __shfl_down(s, 1);
        if (t == 0) totals[blockIdx.x] = s;
    }
}

// one thread: the block prefix in ascending order, the first block whose inclusive prefix exceeds u * total, then an ascending
// scan inside it from the block's exclusive prefix
__global__ void pick_scan_kernel(const float* __restrict__ w, long long N, const double* __restrict__ totals, long long nb, double u,
                                 long long* __restrict__ pick) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double total = 0.0;
    for (long long b = 0; b < nb; ++b) total += totals[b];
    long long at = (long long)(u * (double)N);
    at = at < 0 ? 0 : (at >= N ? N - 1 : at);
    if (total > 0.0) {
        const double target = u * total;
        double before = 0.0;
        long long b = 0;
        for (; b < nb - 1; ++b) {
            if (before + totals[b] > target) break;
            before += totals[b];
        }
        const long long i0 = b * PICK_BLOCK, i1 = i0 + PICK_BLOCK < N ? i0 + PICK_BLOCK : N;
        double run = before;
        long long last = i1 - 1;                           // (no element exceeds by rounding: the block's last positive weight)
        bool found = false;
        for (long long i = i0; i < i1 && !found; ++i) {
            const float wi = w[i];
            run += (double)wi;
            if (wi > 0.f) last = i;
            if (run > target) {
                at = i;
                found = true;
            }
        }
        if (!found) at = last;
    }
    *pick = at;
}

__global__ __launch_bounds__(256) void contingency_kernel(const int32_t* __restrict__ a, const int32_t* __restrict__ b, long long N,
                                                          int na, int nb, unsigned long long* __restrict__ table,
                                                          int32_t* __restrict__ flag) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int x = a[i], y = b[i];
    if (x < 0 || x >= na || y < 0 || y >= nb) {
        atomicOr(flag, 1);
        return;
    }
    atomicAdd(&table[(long long)x * nb + y], 1ull);
}

// rows per segment: the caller's, or equally long segments of whole 128-row tiles, one per resident workgroup at the most
inline long long kmeans_seg_len(long long N, long long seg_rows) {
    if (seg_rows > 0) return seg_rows;
    const long long tiles = (N + 127) / 128;
    const long long slots = resident_workgroups();
    const long long S = tiles < slots ? tiles : slots;
    return (tiles + S - 1) / S * 128;
}

struct KmeansWs {
    long long S, parts, off_inertia, off_shift, off_cnt, off_changed, bytes;
};

inline KmeansWs kmeans_layout(long long N, int L, int k, long long seg_rows) {
    KmeansWs w;
    const long long seg_len = kmeans_seg_len(N, seg_rows);
    w.S = (N + seg_len - 1) / seg_len;
    w.parts = ((long long)k * L + 255) / 256;
    w.off_inertia = 8 * w.S * k * L;
    w.off_shift = w.off_inertia + 8 * w.S;
    w.off_cnt = w.off_shift + 8 * w.parts;
    w.off_changed = w.off_cnt + 4 * w.S * k;
    w.bytes = (w.off_changed + 4 * w.S + 15) / 16 * 16;
    return w;
}

inline bool kmeans_args_ok(long long N, int L, int k, long long seg_rows) {
    return N >= 1 && N < 2147483647ll && L >= 1 && k >= 1 && k <= KM_KMAX && k <= N && seg_rows >= 0 && seg_rows % 128 == 0;
}

}  // namespace

extern "C" long long jamie_kmeans_workspace(long long N, int L, int k, long long seg_rows) {
    if (!kmeans_args_ok(N, L, k, seg_rows)) return 0;
    return kmeans_layout(N, L, k, seg_rows).bytes;
}

extern "C" int jamie_kmeans_step(const float* X, long long N, int L, float* C, int k, int32_t* labels, float* minq, double* sums,
                                 long long* counts, double* stats, int32_t* state, double tol_abs, int max_iter, int update,
                                 long long seg_rows, void* ws, long long ws_bytes, void* stream) {
    JAMIE_ARG(N >= 1 && N < 2147483647ll && L >= 1, "1 <= N < 2^31, L >= 1");
    JAMIE_ARG(k >= 1 && k <= KM_KMAX && k <= N, "1 <= k <= min(N, 1024)");
    JAMIE_ARG(seg_rows >= 0 && seg_rows % 128 == 0, "seg_rows is 0 or a positive multiple of 128");
    JAMIE_ARG(X && C && labels && counts && stats && state && ws, "null pointer");
    JAMIE_ARG(max_iter >= 1 && tol_abs >= 0.0, "max_iter >= 1, tol_abs >= 0");
    const KmeansWs w = kmeans_layout(N, L, k, seg_rows);
    JAMIE_ARG(ws_bytes >= w.bytes, "workspace smaller than jamie_kmeans_workspace(N, L, k, seg_rows)");
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)ws;
    double* slab = (double*)base;
    double* seg_inertia = (double*)(base + w.off_inertia);
    double* shift_part = (double*)(base + w.off_shift);
    int* cnt_slab = (int*)(base + w.off_cnt);
    int* seg_changed = (int*)(base + w.off_changed);
    const int vec = (L % 4 == 0) && aligned16(X) && aligned16(C);
    const long long seg_len = kmeans_seg_len(N, seg_rows);
    if ((long long)k * L <= TAB_MAX)
        hipLaunchKernelGGL(kmeans_step_kernel<true>, dim3((unsigned)w.S), dim3(256), 0, st, X, N, L, vec, (const float*)C, k, labels,
                           minq, seg_len, slab, seg_inertia, cnt_slab, seg_changed, (const int32_t*)state);
    else
        hipLaunchKernelGGL(kmeans_step_kernel<false>, dim3((unsigned)w.S), dim3(256), 0, st, X, N, L, vec, (const float*)C, k, labels,
                           minq, seg_len, slab, seg_inertia, cnt_slab, seg_changed, (const int32_t*)state);
    hipLaunchKernelGGL(kmeans_reduce_kernel, dim3((unsigned)w.parts), dim3(256), 0, st, (const double*)slab, (const int*)cnt_slab, w.S,
                       k, L, C, update, sums, counts, shift_part, (const int32_t*)state);
    hipLaunchKernelGGL(kmeans_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)seg_inertia, (const int*)seg_changed, w.S,
                       (const double*)shift_part, (int)w.parts, (const long long*)counts, k, tol_abs, max_iter, stats, state);
    return jamie_launch_status("jamie_kmeans_step");
}

extern "C" int jamie_kmeans_min_update(const float* X, long long N, int L, const long long* row, float* centre, float* minq,
                                       int first, void* stream) {
    JAMIE_ARG(N >= 1 && N < 2147483647ll && L >= 1, "1 <= N < 2^31, L >= 1");
    JAMIE_ARG(X && row && minq, "null pointer");
    hipLaunchKernelGGL(kmeans_min_update_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, X, N, L, row,
                       centre, minq, first);
    return jamie_launch_status("jamie_kmeans_min_update");
}

extern "C" int jamie_weighted_pick(const float* w, long long N, double u, long long* pick, void* ws, long long ws_bytes,
                                   void* stream) {
    JAMIE_ARG(N >= 1 && N < 2147483647ll, "1 <= N < 2^31");
    JAMIE_ARG(u >= 0.0 && u < 1.0, "0 <= u < 1");
    JAMIE_ARG(w && pick && ws, "null pointer");
    const long long nb = (N + PICK_BLOCK - 1) / PICK_BLOCK;
    JAMIE_ARG(ws_bytes >= 8 * nb, "workspace smaller than 8 ceil(N / 1024) bytes");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(pick_totals_kernel, dim3((unsigned)nb), dim3(256), 0, st, w, N, (double*)ws);
    hipLaunchKernelGGL(pick_scan_kernel, dim3(1), dim3(64), 0, st, w, N, (const double*)ws, nb, u, pick);
    return jamie_launch_status("jamie_weighted_pick");
}

extern "C" int jamie_contingency(const int32_t* a, const int32_t* b, long long N, int na, int nb, long long* table, int32_t* flag,
                                 void* stream) {
    JAMIE_ARG(N >= 1 && na >= 1 && nb >= 1, "N, na, nb >= 1");
    JAMIE_ARG(a && b && table && flag, "null pointer");
    hipLaunchKernelGGL(contingency_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, b, N, na, nb,
                       (unsigned long long*)table, flag);
    return jamie_launch_status("jamie_contingency");
}

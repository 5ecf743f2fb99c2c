// Sorting fp32 columns as order-preserving uint32 keys, feature-major, shared by csrc/imputation.hip (AUROC) and csrc/markers.hip
// (rank sums): the key map, binary searches in a sorted column, a bitonic sort of CHUNK keys per workgroup in LDS and rank-merge
// passes between two buffers until a column of Npad keys (a multiple of CHUNK; padding: the sentinel, past every finite value) is
// one ascending run.
#pragma once
#include "common.h"

namespace {

constexpr int CHUNK = 4096;            // keys a workgroup sorts in LDS: 16 KB (jamie_amd/imputation.py CHUNK)
constexpr uint32_t SENTINEL = 0xFFFFFFFFu;

// fp32 -> uint32 with the order of the floats; -0.0 takes the key of +0.0
__device__ __forceinline__ uint32_t order_key(float x) {
    uint32_t u = __builtin_bit_cast(uint32_t, x);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// first index in the sorted a[0, n) whose key is >= key: every lane of a wave that searches the same n makes the same number of
// steps.  The first index whose key is > key is lower_bound(key + 1): the keys are integers
__device__ __forceinline__ long long lower_bound(const uint32_t* __restrict__ a, long long n, uint32_t key) {
    long long base = 0;
    while (n > 1) {
        const long long half = n >> 1;
        base += a[base + half - 1] < key ? half : 0;
        n -= half;
    }
    return base + ((n == 1 && a[base] < key) ? 1 : 0);
}
__device__ __forceinline__ long long upper_bound(const uint32_t* __restrict__ a, long long n, uint32_t key) {
    return key == SENTINEL ? n : lower_bound(a, n, key + 1);
}

// lower_bound(key) + lower_bound(key + 1), key below the sentinel: the two searches side by side, two loads in flight per step
__device__ __forceinline__ long long rank2(const uint32_t* __restrict__ a, long long n, uint32_t key) {
    long long b0 = 0, b1 = 0;
    const uint32_t k1 = key + 1;
    while (n > 1) {
        const long long half = n >> 1;
        const uint32_t v0 = a[b0 + half - 1], v1 = a[b1 + half - 1];
        b0 += v0 < key ? half : 0;
        b1 += v1 < k1 ? half : 0;
        n -= half;
    }
    if (n == 1) {
        const uint32_t v0 = a[b0], v1 = a[b1];
        b0 += v0 < key ? 1 : 0;
        b1 += v1 < k1 ? 1 : 0;
    }
    return b0 + b1;
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// one workgroup: CHUNK keys of one feature, sorted ascending in LDS (bitonic network)
__global__ __launch_bounds__(256) void chunk_sort_kernel(uint32_t* __restrict__ keys, long long Npad) {
    __shared__ uint32_t s[CHUNK];
    uint32_t* g = keys + (long long)blockIdx.y * Npad + (long long)blockIdx.x * CHUNK;
    for (int t = threadIdx.x; t < CHUNK / 4; t += 256)
        reinterpret_cast<uint4*>(s)[t] = reinterpret_cast<const uint4*>(g)[t];
    __syncthreads();
    for (int k = 2; k <= CHUNK; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < CHUNK / 2; t += 256) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const uint32_t a = s[i], b = s[i + j];
                const bool up = (i & k) == 0;
                if ((a > b) == up) {
                    s[i] = b;
                    s[i + j] = a;
                }
            }
            __syncthreads();
        }
    for (int t = threadIdx.x; t < CHUNK / 4; t += 256) reinterpret_cast<uint4*>(g)[t] = reinterpret_cast<const uint4*>(s)[t];
}

// Merge path: how many keys of A are among the first `diag` keys of merge(A, B), A first on ties.  "A[m] <= B[diag - 1 - m]" holds
// for every m below the answer and for none from it on; the 64 lanes of a wave test 64 evenly spaced m per step, so runs of 2^19
// keys take 5 steps.  The whole wave calls it; the result is the same in every lane.
__device__ __forceinline__ long long merge_split(const uint32_t* __restrict__ A, long long nA, const uint32_t* __restrict__ B,
                                                 long long nB, long long diag, int lane) {
    long long lo = diag > nB ? diag - nB : 0, hi = diag < nA ? diag : nA;
    while (lo < hi) {
        const long long step = (hi - lo + 63) >> 6;
        const long long mid = lo + lane * step;
        const bool before = mid < hi && A[mid] <= B[diag - 1 - mid];
        const int cnt = __popcll(__ballot(before));
        if (cnt == 0) {
            hi = lo;
        } else {
            const long long m = lo + (cnt - 1) * step;         // the last m tested that holds
            lo = m + 1;
            hi = hi < m + step ? hi : m + step;
        }
    }
    return lo;
}

// One pass over runs of R keys, merged pairwise; a last run without a partner is copied.  A workgroup puts out MERGE_T consecutive
// keys of a merged pair: two waves find where that window starts and ends in both runs (merge_split), the two slices -- MERGE_T
// keys together -- go to LDS, and there every key is ranked in the other slice: a key of the left slice at i goes to
// i + lower_bound(right slice), a key of the right slice at j to j + upper_bound(left slice).  Global reads and writes are contiguous.
constexpr int MERGE_T = 2048;
__global__ __launch_bounds__(256) void rank_merge_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, long long Npad,
                                                         long long R) {
    __shared__ uint32_t S[MERGE_T], O[MERGE_T];
    __shared__ long long split[2];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long og = (long long)blockIdx.x * MERGE_T;      // (R and the runs' lengths are multiples of CHUNK >= MERGE_T:
    const uint32_t* a = src + (long long)blockIdx.y * Npad;    //  a window lies in one pair)
    uint32_t* o = dst + (long long)blockIdx.y * Npad;
    const long long base = og / (2 * R) * (2 * R), b0 = base + R;
    if (b0 >= Npad) {                                          // (the same in every thread)
        for (int t = threadIdx.x; t < MERGE_T; t += 256) o[og + t] = a[og + t];
        return;
    }
    const long long nB = Npad - b0 < R ? Npad - b0 : R;
    const uint32_t* A = a + base;
    const uint32_t* B = a + b0;
    const long long d0 = og - base;
    if (w < 2) {
        const long long s = merge_split(A, R, B, nB, d0 + (long long)w * MERGE_T, lane);
        if (lane == 0) split[w] = s;
    }
    __syncthreads();
    const long long a0 = split[0], bb0 = d0 - a0;
    const int na = (int)(split[1] - a0), nb = MERGE_T - na;
    for (int t = threadIdx.x; t < MERGE_T; t += 256) S[t] = t < na ? A[a0 + t] : B[bb0 + (t - na)];
    __syncthreads();
    for (int t = threadIdx.x; t < MERGE_T; t += 256) {
        const uint32_t key = S[t];
        const int to = t < na ? t + (int)lower_bound(S + na, nb, key) : (t - na) + (int)upper_bound(S, na, key);
        O[to] = key;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < MERGE_T; t += 256) o[og + t] = O[t];
}

inline long long pad_to_chunk(long long N) { return (N + CHUNK - 1) / CHUNK * CHUNK; }

// the sort of `cols` columns of Npad keys in `a` (the key pass has filled it), with `b` as the second buffer: the chunk sort when
// last_stage >= 2, the merge passes when last_stage >= 3.  Returns the buffer that holds the result.
inline uint32_t* sort_columns(uint32_t* a, uint32_t* b, long long Npad, int cols, int last_stage, hipStream_t st) {
    if (last_stage >= 2)
        hipLaunchKernelGGL(chunk_sort_kernel, dim3((unsigned)(Npad / CHUNK), (unsigned)cols), dim3(256), 0, st, a, Npad);
    if (last_stage >= 3)
        for (long long R = CHUNK; R < Npad; R *= 2) {
            hipLaunchKernelGGL(rank_merge_kernel, dim3((unsigned)(Npad / MERGE_T), (unsigned)cols), dim3(256), 0, st, a, b, Npad, R);
            uint32_t* t = a;
            a = b;
            b = t;
        }
    return a;
}

}  // namespace

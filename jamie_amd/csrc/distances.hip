// Stage A of the correspondence path on the MI355X: the cell x cell distance matrices of `compute_distances` (reference
// jamie.py:839-890) for the euclidean modes, the geodesic mode (kNN graph + all-pairs shortest paths, unioncom's
// geodesic_distances, jamie_amd/utilities.py), the correlation family (cosine / correlation / pearson: the euclidean Gram pass on
// unit rows, row_normalise_kernel + tile_pair_kernel<3>) and the L1 family (manhattan / chebyshev: absdiff_kernel, all pairs by
// direct difference).  The host side (jamie_amd/distances.py) centres the columns with
// jamie_col_stats / jamie_standardise and forms the Gram matrix G = Xc Xc^T on jamie_gemm_f32_cfg (configuration 17, the exact
// fp32 pipe) straight into the N x N output; everything below works in that one N x N buffer (row-major, ld = N).
//
// Padding: the tiled kernels treat rows / columns >= N as +inf (loads return +inf, stores are skipped) instead of storing a
// padded matrix: a +inf row or column never shortens a path, so the result on the first N rows and columns is the padded
// algorithm's, and no copy is needed to drop the padding.
#include "common.h"

#define DIST_PT 64          // tile of the pairwise (tile pair) passes
#define FW_T 128            // Floyd-Warshall block
#define FW_KC 32            // phase 3: k-chunk staged in LDS
#define FW_LDS_LD 34        // ... its row stride in floats (8-byte reads of 16 consecutive rows hit 32 distinct banks)
#define TOPK_MAX 1024       // largest per-row K of jamie_knn_topk

typedef float jf2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float d_inf() { return __builtin_inff(); }

// ------------------------------------------------------------------------------------------------
// squared row norms of the centred data (fp32, the same rounding class as the Gram entries they meet)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void row_sqnorm_kernel(const float* __restrict__ X, long long N, int d, float* __restrict__ out) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= N) return;
    const float* x = X + row * d;
    float s = 0.f;
    for (int c = lane; c < d; c += 64) s = fmaf(x[c], x[c], s);
    s = wave_sum(s);
    if (lane == 0) out[row] = s;
}

// ------------------------------------------------------------------------------------------------
// Tile-pair passes over the N x N buffer: workgroup (I, J), I <= J, owns the tiles (I, J) and (J, I) and reads both before it
// writes either, so the pass runs in place and its output is exactly symmetric.
//   MODE 0: Gram -> euclidean, D = sqrt(q), q = max(n_i + n_j - 2 G_ij, 0), diagonal exactly 0 (G_ij read from the upper triangle)
//   MODE 1: Gram -> squared euclidean, D = q
//   MODE 2: D = min(D, D^T); partial[blk] = largest finite value of the two tiles (0 if none)
//   MODE 3: Gram of (column-centred) unit rows -> D = scale * q (1 - u.v = |u - v|^2 / 2: cosine and correlation distance are
//           q / 2, JAMIE's pearson q / 4); 1 off the diagonal where either row is a zero row (rownorm == 0: sklearn's cosine
//           leaves a zero row zero)
// Modes 0 / 1 / 3 recompute q by direct difference, sum_c (x_ic - x_jc)^2 in fp32, where cancellation dominates: q < DIST_TAU (n_i + n_j).
// n (row_sqnorm_kernel) and G (the MFMA GEMM) round in different orders, so q carries an error of c u (n_i + n_j), u = 2^-24, c ~ 1
// (a few at d = 2000): on (near-)duplicate cells it swamps q.  A pair that keeps the Gram form has q >= tau s (s = n_i + n_j), so
// |dD| <= c u s / (2 sqrt(q)) <= c u sqrt(s / tau) / 2; centred data has, for every i, a j with x_i . x_j <= 0, so
// max D^2 >= max n >= s / 2, and |dD| <= c u / sqrt(2 tau) max D = 1.35e-6 c max D at tau = 2^-10 (the 1e-5 max D contract holds for
// c <= 7).  Gaussian data recomputes nothing (q ~ s); exact duplicates come out exactly 0.
// ------------------------------------------------------------------------------------------------
#define DIST_TAU 0x1p-10f

template <int MODE>
__global__ __launch_bounds__(256) void tile_pair_kernel(float* D, long long N, const float* __restrict__ sqn, const float* __restrict__ X,
                                                        int d, float* partial, float scale, const float* __restrict__ rownorm) {
    const int I = blockIdx.y, J = blockIdx.x;
    const int nt = gridDim.x;
    __shared__ float sA[DIST_PT][DIST_PT + 1], sB[DIST_PT][DIST_PT + 1];
    __shared__ float red[4];
    if (I > J) {
        if (MODE == 2 && threadIdx.x == 0) partial[(long long)I * nt + J] = 0.f;
        return;
    }
    const long long i0 = (long long)I * DIST_PT, j0 = (long long)J * DIST_PT;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int r = ty; r < DIST_PT; r += 4) {
        const long long i = i0 + r, j = j0 + tx;
        sA[r][tx] = (i < N && j < N) ? D[i * N + j] : 0.f;                 // tile (I, J), row r col tx
        const long long i2 = j0 + r, j2 = i0 + tx;
        sB[r][tx] = (i2 < N && j2 < N) ? D[i2 * N + j2] : 0.f;             // tile (J, I), row r col tx
    }
    __syncthreads();
    float mx = 0.f;
    for (int r = ty; r < DIST_PT; r += 4) {                                // (r, hence i, is uniform in a wave; j = j0 + lane)
        const int c = tx;
        const long long i = i0 + r, j = j0 + c;
        const bool ok = i < N && j < N;
        float v = 0.f;
        if (MODE == 2) {
            if (ok) {
                v = fminf(sA[r][c], sB[c][r]);                             // D_ij, D_ji
                if (v < d_inf()) mx = fmaxf(mx, v);
            }
        } else {
            float q = 0.f;
            bool redo = false;
            if (ok) {
                const float g = (I < J || r <= c) ? sA[r][c] : sA[c][r];   // G of the upper triangle
                q = fmaxf(sqn[i] + sqn[j] - 2.f * g, 0.f);
                redo = i != j && q < DIST_TAU * (sqn[i] + sqn[j]);
                if (i == j) q = 0.f;
            }
            // the wave recomputes its flagged pairs one at a time, 64 lanes over the d columns (fixed order: deterministic)
            for (unsigned long long m = __ballot(redo); m; m &= m - 1) {
                const int l = __builtin_ctzll(m);
                const float* xi = X + i * d;
                const float* xj = X + (j0 + l) * d;
                float s = 0.f;
                for (int cc = tx; cc < d; cc += 64) {
                    const float t = xi[cc] - xj[cc];
                    s = fmaf(t, t, s);
                }
                s = wave_sum(s);
                if (tx == l) q = s;
            }
            v = MODE == 0 ? sqrtf(q) : q;
            if (MODE == 3) {
                v = scale * q;
                if (ok && i != j && (rownorm[i] == 0.f || rownorm[j] == 0.f)) v = 1.f;
            }
        }
        if (!ok) continue;
        D[i * N + j] = v;
        if (I != J) D[j * N + i] = v;
    }
    if (MODE == 2) {
        for (int o = 1; o < 64; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
        if (tx == 0) red[ty] = mx;
        __syncthreads();
        if (threadIdx.x == 0) partial[(long long)I * nt + J] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    }
}

// one workgroup: maxv[0] = max of the partials (a fixed reduction tree)
__global__ __launch_bounds__(256) void max_reduce_kernel(const float* __restrict__ partial, long long n, float* maxv) {
    __shared__ float red[256];
    float m = 0.f;
    for (long long i = threadIdx.x; i < n; i += 256) m = fmaxf(m, partial[i]);
    red[threadIdx.x] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) maxv[0] = red[0];
}

// unreachable pairs (+inf) -> 2 * largest finite value (0 when nothing is finite: 2 * 0)
__global__ __launch_bounds__(256) void fill_unreachable_kernel(float* D, long long n, const float* __restrict__ maxv) {
    const float fill = 2.f * maxv[0];
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256)
        if (!(D[e] < d_inf())) D[e] = fill;
}

// ------------------------------------------------------------------------------------------------
// Unit rows for the correlation family (the host side column-centres them before the Gram pass: |u - v|^2 does not change under a
// shift, and all-positive rows such as counts are nearly parallel -- G ~ 1 everywhere, where a d = 2000 fma chain loses 1e-5):
// out[i, :] = (x_i - m_i) / |x_i - m_i| as fp32, m_i = the row's mean (centre = 1) or 0.
// Mean, norm and the quotient are taken in fp64 with one rounding to fp32 at the store (as jamie_col_stats / jamie_standardise do
// for columns).  norm[i] = that norm as fp32, exactly 0 for a row the host cannot normalise -- a zero row, or with centre = 1 a
// constant row (every entry equal; tested on the entries, not on the rounded norm) -- and such a row is written as zeros.
// One wave per row, fixed reduction order: deterministic.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum_f64(double v) {
    for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);       // (lane l and lane l ^ o add the same two numbers: uniform result)
    return v;
}

template <typename T>
__global__ __launch_bounds__(256) void row_normalise_kernel(const T* __restrict__ X, long long N, int d, int centre,
                                                            float* __restrict__ out, float* __restrict__ norm) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= N) return;
    const T* x = X + row * d;
    double mean = 0.0;
    bool flat = false;
    if (centre) {
        const T x0 = x[0];
        double s = 0.0;
        bool differs = false;
        for (int c = lane; c < d; c += 64) {
            s += (double)x[c];
            differs |= x[c] != x0;
        }
        mean = wave_sum_f64(s) / (double)d;
        flat = __ballot(differs) == 0ull;
    }
    double q = 0.0;
    for (int c = lane; c < d; c += 64) {
        const double t = (double)x[c] - mean;
        q += t * t;
    }
    const double nrm = flat ? 0.0 : sqrt(wave_sum_f64(q));
    float* o = out + row * d;
    for (int c = lane; c < d; c += 64) o[c] = nrm > 0.0 ? (float)(((double)x[c] - mean) / nrm) : 0.f;
    if (lane == 0) norm[row] = nrm > 0.0 ? fmaxf((float)nrm, 0x1p-126f) : 0.f;      // (a tiny norm must not read as a zero row)
}

// ------------------------------------------------------------------------------------------------
// L1 family: D_ij = sum_c |x_ic - x_jc| (OP 0) or max_c |x_ic - x_jc| (OP 1) over all pairs of one [N, d] fp32 matrix, by direct
// difference, written straight into the N x N output.  The tile shape is the pair tile of csrc/metrics.hip: 256 threads own
// 128 x 128 pairs, a thread 8 x 8 of them (rows (r / 4) * 64 + ty * 4 + r % 4, columns (s / 4) * 64 + tx * 4 + s % 4); both operands
// are staged feature-major in LDS, AD_KC = 32 features per trip, and read back as ds_read_b128 (rows: broadcast; columns: 16
// contiguous 16-byte slots).  Per pair and feature: v_sub_f32 + v_add_f32 (v_max_f32) with the |.| source modifier -- VALU-issue
// bound, hence the two workgroups per CU of the launch bounds.
// One chain per pair in ascending c; OP 0 sums every trip into a fresh partial and adds the partial to the total (chunks of 32:
// the error of a d = 2000 sum drops from 2.7e-6 to 4.8e-7 max D).  |a - b| == |b - a| and x - x == 0, so the diagonal is exactly 0
// and the matrix exactly symmetric; features past d and rows past N are staged as 0 and add |0 - 0| = 0.  Exact on data whose
// differences and sums are fp32 numbers (integers).
// Only the tiles I <= J are computed.  A tile leaves through LDS, 64 rows at a time, so that the stores of both the tile and its
// mirror image walk along rows of D: the direct half-tile is written row-major (8 lanes of a ds_write_b128 group: 32 contiguous
// dwords), the mirror half-tile with its LDS rows permuted, local column tx * 4 + k in LDS row k * 16 + tx, so that the 8 lanes of
// a group are AD_LD = 132 dwords apart: banks 4 tx .. 4 tx + 3, conflict-free (unpermuted they would be 528 apart: two banks of 8).
// ------------------------------------------------------------------------------------------------
#define AD_KC 32
#define AD_T 128
#define AD_LD (AD_T + 4)
#define AD_LAUNCH_WORK 4000000000000ll      // pair-features per launch (a fraction of a second)

// rows [r0, r0 + 128) x features [c0, c0 + 32) of X [N, d] -> S[feature][row], zero where the row or the feature does not exist
__device__ __forceinline__ void ad_stage(const float* __restrict__ X, long long N, long long r0, int d, int c0, bool vec,
                                         float* __restrict__ S) {
    for (int s = threadIdx.x; s < AD_T * (AD_KC / 4); s += 256) {
        const int r = s >> 3, c = c0 + (s & 7) * 4;
        const long long gr = r0 + r;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (gr < N) {
            const float* p = X + gr * d + c;
            if (vec && c + 3 < d) {
                const float4 x = *reinterpret_cast<const float4*>(p);
                v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (c + k < d) v[k] = p[k];
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) S[((s & 7) * 4 + k) * AD_LD + r] = v[k];
    }
}

// 64 x 128 floats of LDS (row stride AD_LD) -> rows gi0 + row(p), columns gj0 .. gj0 + 127 of D; a wave stores 64 consecutive floats
template <bool PERMUTED>
__device__ __forceinline__ void ad_store_rows(const float* __restrict__ S, float* __restrict__ D, long long N, long long gi0,
                                              long long gj0) {
    for (int e = threadIdx.x; e < 64 * AD_T; e += 256) {
        const int p = e >> 7, c = e & 127;
        const long long gi = gi0 + (PERMUTED ? (p & 15) * 4 + (p >> 4) : p), gj = gj0 + c;
        if (gi < N && gj < N) D[gi * N + gj] = S[p * AD_LD + c];
    }
}

// acc (+ or max)= |a - b|.  The accumulate is spelled out: from `acc + fabsf(t)` hipcc's SLP vectoriser makes v_pk_add_f32 pairs, which
// have no |.| modifier (two v_and_b32 beside every packed add) and issue at half the rate of a plain VALU instruction: 1.5 times the
// issue cycles; from fmaxf it adds a canonicalising v_max_f32 per value.
template <int OP>
__device__ __forceinline__ void ad_step(float& acc, float a, float b) {
    const float t = a - b;
    if (OP == 0) asm("v_add_f32_e64 %0, |%1|, %0" : "+v"(acc) : "v"(t));
    else asm("v_max_f32_e64 %0, |%1|, %0" : "+v"(acc) : "v"(t));
}

template <int OP>
__global__ __launch_bounds__(256, 2) void absdiff_kernel(const float* __restrict__ X, long long N, int d, int vec, long long tile_i0,
                                                         float* __restrict__ D) {
    const long long I = tile_i0 + blockIdx.y, J = blockIdx.x;
    if (J < I) return;
    __shared__ __attribute__((aligned(16))) float smem[2 * AD_KC * AD_LD];      // the staged operands, then 64 x AD_LD of output
    float* Xs = smem;
    float* Ys = I == J ? smem : smem + AD_KC * AD_LD;                           // (a diagonal tile stages its rows once)
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const long long i0 = I * AD_T, j0 = J * AD_T;
    float acc[8][8];
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
        for (int s = 0; s < 8; ++s) acc[r][s] = 0.f;
    for (int c0 = 0; c0 < d; c0 += AD_KC) {
        __syncthreads();                                   // the last trip's reads are done
        ad_stage(X, N, i0, d, c0, vec != 0, Xs);
        if (I != J) ad_stage(X, N, j0, d, c0, vec != 0, Ys);
        __syncthreads();
        const int rest = (d - c0 + 3) & ~3;
        const int kc = rest < AD_KC ? rest : AD_KC;
        float part[8][8];
        if (OP == 0) {
#pragma unroll
            for (int r = 0; r < 8; ++r)
#pragma unroll
                for (int s = 0; s < 8; ++s) part[r][s] = 0.f;
        }
#pragma unroll 2
        for (int c = 0; c < kc; ++c) {
            float a[8], b[8];
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const float4 x = *reinterpret_cast<const float4*>(&Xs[c * AD_LD + m * 64 + ty * 4]);
                a[m * 4] = x.x; a[m * 4 + 1] = x.y; a[m * 4 + 2] = x.z; a[m * 4 + 3] = x.w;
                const float4 y = *reinterpret_cast<const float4*>(&Ys[c * AD_LD + m * 64 + tx * 4]);
                b[m * 4] = y.x; b[m * 4 + 1] = y.y; b[m * 4 + 2] = y.z; b[m * 4 + 3] = y.w;
            }
#pragma unroll
            for (int r = 0; r < 8; ++r)
#pragma unroll
                for (int s = 0; s < 8; ++s) ad_step<OP>(OP == 0 ? part[r][s] : acc[r][s], a[r], b[s]);
        }
        if (OP == 0) {
#pragma unroll
            for (int r = 0; r < 8; ++r)
#pragma unroll
                for (int s = 0; s < 8; ++s) acc[r][s] += part[r][s];
        }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {                          // rows h * 64 .. of the tile (I, J)
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int m = 0; m < 2; ++m)
                *reinterpret_cast<float4*>(&smem[(ty * 4 + r) * AD_LD + m * 64 + tx * 4]) =
                    make_float4(acc[h * 4 + r][m * 4], acc[h * 4 + r][m * 4 + 1], acc[h * 4 + r][m * 4 + 2], acc[h * 4 + r][m * 4 + 3]);
        __syncthreads();
        ad_store_rows<false>(smem, D, N, i0 + h * 64, j0);
    }
    if (I == J) return;
#pragma unroll
    for (int m = 0; m < 2; ++m) {                          // columns m * 64 .. of the tile = rows of the tile (J, I)
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int h = 0; h < 2; ++h)
                *reinterpret_cast<float4*>(&smem[(k * 16 + tx) * AD_LD + h * 64 + ty * 4]) =
                    make_float4(acc[h * 4][m * 4 + k], acc[h * 4 + 1][m * 4 + k], acc[h * 4 + 2][m * 4 + k], acc[h * 4 + 3][m * 4 + k]);
        __syncthreads();
        ad_store_rows<true>(smem, D, N, j0 + m * 64, i0);
    }
}

// ------------------------------------------------------------------------------------------------
// Per-row top-K: the K - 1 smallest off-diagonal entries of row i, ascending by (value, column), behind the cell itself in
// slot 0.  Non-negative fp32 values order like their bit patterns: the key of entry j is (bits(D_ij), j), and an MSB-first
// radix select on it (8-bit digits of the value bits, starting below the prefix the row's minimum and maximum share, then
// 8-bit digits of the column index to break ties) finds the selected set; it stops as soon as the bucket that holds the
// K-th key is taken whole.  Only the survivors are sorted (bitonic, in LDS).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long dist_key(unsigned v, unsigned j) { return ((unsigned long long)v << 32) | j; }

__global__ __launch_bounds__(256) void topk_kernel(const float* __restrict__ D, long long N, int K, int32_t* __restrict__ idx) {
    const long long i = blockIdx.x;
    const unsigned* row = reinterpret_cast<const unsigned*>(D + i * N);
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    __shared__ unsigned hist[256];
    __shared__ unsigned wred[2][4];
    __shared__ unsigned long long keys[TOPK_MAX];
    __shared__ unsigned sel_count;
    __shared__ unsigned s_bucket, s_below;
    const int need0 = K - 1;                                   // off-diagonal neighbours
    if (need0 <= 0) {
        if (t == 0) idx[i * K] = (int32_t)i;
        return;
    }
    // ---- row minimum / maximum off the diagonal ----
    unsigned mn = 0xFFFFFFFFu, mxv = 0u;
    for (long long j = t; j < N; j += 256) {
        if (j == i) continue;
        const unsigned v = row[j];
        mn = min(mn, v);
        mxv = max(mxv, v);
    }
    for (int o = 1; o < 64; o <<= 1) {
        mn = min(mn, (unsigned)__shfl_xor((int)mn, o));
        mxv = max(mxv, (unsigned)__shfl_xor((int)mxv, o));
    }
    if (lane == 0) { wred[0][w] = mn; wred[1][w] = mxv; }
    __syncthreads();
    mn = min(min(wred[0][0], wred[0][1]), min(wred[0][2], wred[0][3]));
    mxv = max(max(wred[1][0], wred[1][1]), max(wred[1][2], wred[1][3]));
    // digits: value bits [hb .. 0] (hb = highest bit where min and max differ), then index bits [23 .. 0]
    const unsigned diff = mn ^ mxv;
    const int hb = diff ? 31 - __builtin_clz(diff) : -1;
    unsigned pv = mn & ~(diff ? ((hb == 31) ? 0xFFFFFFFFu : ((2u << hb) - 1u)) : 0u);   // common prefix of every value
    unsigned mv = diff ? ~((hb == 31) ? 0xFFFFFFFFu : ((2u << hb) - 1u)) : 0xFFFFFFFFu;
    unsigned pj = 0, mj = 0;
    int need = need0;
    int hi = hb;                       // current digit's top bit (value bits while hi >= 0, then index bits)
    bool in_index = hb < 0;
    if (in_index) hi = 23;
    // every entry of the row has (v & mv) == pv at this point
    for (;;) {
        const int width = min(8, hi + 1);
        const int lo = hi - width + 1;
        const unsigned dmask = ((1u << width) - 1u);
        hist[t] = 0;
        __syncthreads();
        for (long long j = t; j < N; j += 256) {
            if (j == i) continue;
            const unsigned v = row[j];
            if ((v & mv) != pv || ((unsigned)j & mj) != pj) continue;
            const unsigned dig = in_index ? (((unsigned)j >> lo) & dmask) : ((v >> lo) & dmask);
            atomicAdd(&hist[dig], 1u);
        }
        __syncthreads();
        if (w == 0) {                                           // bucket holding the need-th key: wave scan of 4 bins / lane
            const unsigned c0 = hist[4 * lane], c1 = hist[4 * lane + 1], c2 = hist[4 * lane + 2], c3 = hist[4 * lane + 3];
            const unsigned tot = c0 + c1 + c2 + c3;
            unsigned incl = tot;
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned u = (unsigned)__shfl_up((int)incl, o);
                if (lane >= o) incl += u;
            }
            const unsigned excl = incl - tot;
            if (excl < (unsigned)need && incl >= (unsigned)need) {
                unsigned b = 4 * lane, below = excl;
                if (below + c0 < (unsigned)need) { below += c0; ++b;
                    if (below + c1 < (unsigned)need) { below += c1; ++b;
                        if (below + c2 < (unsigned)need) { below += c2; ++b; } } }
                s_bucket = b;
                s_below = below;
            }
        }
        __syncthreads();
        const unsigned b = s_bucket, below = s_below, cb = hist[b];
        __syncthreads();
        need -= (int)below;
        if (in_index) { pj |= b << lo; mj |= dmask << lo; }
        else { pv |= b << lo; mv |= dmask << lo; }
        if (cb == (unsigned)need) break;                        // the bucket is taken whole
        if (!in_index && lo == 0) { in_index = true; hi = 23; }
        else hi = lo - 1;
        if (in_index && hi < 0) break;                          // (unreachable: keys are unique)
    }
    // ---- collect: every key whose determined digits are <= the prefix ----
    int P2 = 1;
    while (P2 < need0) P2 <<= 1;
    for (int s = t; s < P2; s += 256) keys[s] = ~0ull;        // (an unfilled slot would read as column -1, never as garbage)
    if (t == 0) sel_count = 0;
    __syncthreads();
    for (long long j = t; j < N; j += 256) {
        if (j == i) continue;
        const unsigned v = row[j];
        const unsigned a = v & mv, bj = (unsigned)j & mj;
        if (a < pv || (a == pv && bj <= pj)) {
            const unsigned s = atomicAdd(&sel_count, 1u);
            if (s < (unsigned)need0) keys[s] = dist_key(v, (unsigned)j);
        }
    }
    __syncthreads();
    for (int k = 2; k <= P2; k <<= 1) {                         // bitonic sort, ascending
        for (int jj = k >> 1; jj > 0; jj >>= 1) {
            for (int s = t; s < P2; s += 256) {
                const int p = s ^ jj;
                if (p > s) {
                    const unsigned long long a = keys[s], c = keys[p];
                    const bool up = (s & k) == 0;
                    if ((a > c) == up) { keys[s] = c; keys[p] = a; }
                }
            }
            __syncthreads();
        }
    }
    int32_t* out = idx + i * K;
    for (int s = t; s < K; s += 256) out[s] = s == 0 ? (int32_t)i : (int32_t)(keys[s - 1] & 0xFFFFFFFFull);
}

// exact edge weights: w[i, s] = sqrt(sum_c (x_ic - x_jc)^2) in fp32, j = idx[i, s]; one wave per edge
__global__ __launch_bounds__(256) void knn_weight_kernel(const float* __restrict__ X, long long N, int d, const int32_t* __restrict__ idx,
                                                         int K, float* __restrict__ wout) {
    const long long e = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (e >= N * K) return;
    const long long i = e / K;
    const long long j = idx[e];
    if (j < 0 || j >= N) {
        if (lane == 0) wout[e] = __builtin_nanf("");
        return;
    }
    const float* xi = X + i * d;
    const float* xj = X + j * d;
    float s = 0.f;
    for (int c = lane; c < d; c += 64) {
        const float t = xi[c] - xj[c];
        s = fmaf(t, t, s);
    }
    s = wave_sum(s);
    if (lane == 0) wout[e] = sqrtf(s);
}

// ------------------------------------------------------------------------------------------------
// graph initialisation: D = +inf, diagonal 0; then every kNN edge (i, idx[i, s]), s < k, to (i, j) and (j, i) keeping the smaller
// weight (csgraph's directed=False rule).  Non-negative fp32 values order like their bits: an unsigned atomic min.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void graph_fill_kernel(float* D, long long N) {
    const long long i = blockIdx.x;
    float* row = D + i * N;
    for (long long j = threadIdx.x; j < N; j += 256) row[j] = j == i ? 0.f : d_inf();
}

__global__ __launch_bounds__(256) void graph_scatter_kernel(float* D, long long N, const int32_t* __restrict__ idx,
                                                            const float* __restrict__ wt, int K, int k) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= N * k) return;
    const long long i = e / k, s = e % k;
    const long long j = idx[i * K + s];
    if (j < 0 || j >= N) return;
    const unsigned b = __builtin_bit_cast(unsigned, wt[i * K + s]);
    atomicMin(reinterpret_cast<unsigned*>(D + i * N + j), b);
    atomicMin(reinterpret_cast<unsigned*>(D + j * N + i), b);
}

// ------------------------------------------------------------------------------------------------
// Blocked Floyd-Warshall (Venkataraman et al. 2003), blocks of FW_T = 128.  Round r:
//   phase 1: the diagonal block (r, r) closed on itself;
//   phase 2: the blocks of row r (through the closed diagonal block on the left) and of column r (on the right);
//   phase 3: every other block (i, j): D_ij = min(D_ij, D_ir (min,+) D_rj) -- independent, GEMM-like.
// Phases 1 and 2: 1024 threads, 4 x 4 entries each in registers; step k needs row k and column k of the block being closed,
// which their owners publish into double-buffered LDS rows after step k - 1 (one barrier per step).  Row k and column k do not
// change at step k (D_kk = 0 and weights are >= 0), so every entry sees the values the sequential algorithm would.
// ------------------------------------------------------------------------------------------------
template <int MODE>   // 0: diagonal block, 1: row block (r, b), 2: column block (b, r)
__global__ __launch_bounds__(1024) void fw_phase12_kernel(float* D, long long N, int r) {
    const int b = blockIdx.x;
    if (MODE != 0 && b == r) return;
    __shared__ float diag[MODE == 0 ? 1 : FW_T * FW_T];
    __shared__ float rowb[2][FW_T], colb[2][FW_T];
    const int t = threadIdx.x, tx = t & 31, ty = t >> 5;
    const long long R0 = (long long)(MODE == 2 ? b : r) * FW_T, C0 = (long long)(MODE == 1 ? b : r) * FW_T;
    const long long K0 = (long long)r * FW_T;
    float own[4][4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const long long i = R0 + ty + 32 * m, j = C0 + tx + 32 * n;
            own[m][n] = (i < N && j < N) ? D[i * N + j] : d_inf();
        }
    if (MODE != 0) {
        for (int e = t; e < FW_T * FW_T; e += 1024) {
            const long long i = K0 + (e >> 7), j = K0 + (e & 127);
            diag[e] = (i < N && j < N) ? D[i * N + j] : d_inf();
        }
    }
    // row k / column k of the block being closed -> LDS (owners: ty == k % 32, resp. tx == k % 32; register row / column k / 32,
    // a constant once the q loop below is unrolled: no dynamic register indexing)
#define FW_PUBLISH(Q, KK, BUF)                                                                          \
    do {                                                                                                \
        if (MODE != 2 && ty == (KK)) {                                                                  \
            _Pragma("unroll") for (int n = 0; n < 4; ++n) rowb[BUF][tx + 32 * n] = own[Q][n];           \
        }                                                                                               \
        if (MODE != 1 && tx == (KK)) {                                                                  \
            _Pragma("unroll") for (int m = 0; m < 4; ++m) colb[BUF][ty + 32 * m] = own[m][Q];           \
        }                                                                                               \
    } while (0)
    FW_PUBLISH(0, 0, 0);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        for (int kk = 0; kk < 32; ++kk) {
            const int k = 32 * q + kk, buf = kk & 1;
            float a[4], bb[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) a[m] = MODE == 1 ? diag[(ty + 32 * m) * FW_T + k] : colb[buf][ty + 32 * m];
#pragma unroll
            for (int n = 0; n < 4; ++n) bb[n] = MODE == 2 ? diag[k * FW_T + tx + 32 * n] : rowb[buf][tx + 32 * n];
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int n = 0; n < 4; ++n) own[m][n] = fminf(own[m][n], a[m] + bb[n]);
            if (kk < 31) FW_PUBLISH(q, kk + 1, buf ^ 1);
            else if (q < 3) FW_PUBLISH(q + 1, 0, buf ^ 1);
            __syncthreads();
        }
    }
#undef FW_PUBLISH
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const long long i = R0 + ty + 32 * m, j = C0 + tx + 32 * n;
            if (i < N && j < N) D[i * N + j] = own[m][n];
        }
}

// phase 3: 256 threads per 128 x 128 block, 8 x 8 entries each (rows ty + 16 m, columns tx + 16 n).  The A panel (block (i, r))
// is staged row-major [row][k] and the B panel (block (r, j)) transposed [col][k], so that a thread reads (a_ik, a_i,k+1) and
// (b_kj, b_k+1,j) as float2: one v_pk_add_f32 forms the two candidates of (i, j) and one v_min3_f32 folds both into the entry
// (written min(min(acc, x), y): hipcc matches it to v_min3_f32; min(acc, min(x, y)) came out as a v_min_f32 / v_min3_f32 mix).
__global__ __launch_bounds__(256, 2) void fw_phase3_kernel(float* D, long long N, int r) {
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (bi == r || bj == r) return;
    __shared__ __attribute__((aligned(16))) float sA[FW_T * FW_LDS_LD], sB[FW_T * FW_LDS_LD];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const long long I0 = (long long)bi * FW_T, J0 = (long long)bj * FW_T, K0 = (long long)r * FW_T;
    float acc[8][8];
#pragma unroll
    for (int m = 0; m < 8; ++m)
#pragma unroll
        for (int n = 0; n < 8; ++n) {
            const long long i = I0 + ty + 16 * m, j = J0 + tx + 16 * n;
            acc[m][n] = (i < N && j < N) ? D[i * N + j] : d_inf();
        }
    for (int kc = 0; kc < FW_T; kc += FW_KC) {
#pragma unroll
        for (int q = 0; q < FW_T * FW_KC / 256; ++q) {
            const int e = t + 256 * q;
            {   // A: row e / 32, k e % 32
                const int row = e >> 5, kk = e & 31;
                const long long i = I0 + row, k = K0 + kc + kk;
                sA[row * FW_LDS_LD + kk] = (i < N && k < N) ? D[i * N + k] : d_inf();
            }
            {   // B: k e / 128, column e % 128
                const int kk = e >> 7, col = e & 127;
                const long long k = K0 + kc + kk, j = J0 + col;
                sB[col * FW_LDS_LD + kk] = (k < N && j < N) ? D[k * N + j] : d_inf();
            }
        }
        __syncthreads();
#pragma unroll 2
        for (int k = 0; k < FW_KC; k += 2) {
            jf2 a[8], b[8];
#pragma unroll
            for (int m = 0; m < 8; ++m) a[m] = *reinterpret_cast<const jf2*>(&sA[(ty + 16 * m) * FW_LDS_LD + k]);
#pragma unroll
            for (int n = 0; n < 8; ++n) b[n] = *reinterpret_cast<const jf2*>(&sB[(tx + 16 * n) * FW_LDS_LD + k]);
#pragma unroll
            for (int m = 0; m < 8; ++m)
#pragma unroll
                for (int n = 0; n < 8; ++n) {
                    const jf2 c = a[m] + b[n];
                    acc[m][n] = __builtin_fminf(__builtin_fminf(acc[m][n], c.x), c.y);
                }
        }
        __syncthreads();
    }
#pragma unroll
    for (int m = 0; m < 8; ++m)
#pragma unroll
        for (int n = 0; n < 8; ++n) {
            const long long i = I0 + ty + 16 * m, j = J0 + tx + 16 * n;
            if (i < N && j < N) D[i * N + j] = acc[m][n];
        }
}

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
static inline int dist_tiles(long long N) { return (int)((N + DIST_PT - 1) / DIST_PT); }

extern "C" long long jamie_dist_workspace(long long N) {
    if (N <= 0) return 0;
    const long long nt = dist_tiles(N);
    return nt * nt;
}

extern "C" int jamie_row_sqnorm(const float* X, long long N, int d, float* out, void* stream) {
    JAMIE_ARG(X && out && N > 0 && d > 0, "null pointer / empty");
    hipLaunchKernelGGL(row_sqnorm_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, (hipStream_t)stream, X, N, d, out);
    return jamie_launch_status("jamie_row_sqnorm");
}

extern "C" int jamie_gram_to_distances(float* D, const float* sqnorm, const float* X, long long N, int d, int squared, void* stream) {
    JAMIE_ARG(D && sqnorm && X && N > 0 && N <= (1 << 24) && d > 0, "null pointer / 0 < N <= 2^24 / d > 0");
    const int nt = dist_tiles(N);
    if (squared) hipLaunchKernelGGL(tile_pair_kernel<1>, dim3(nt, nt), dim3(256), 0, (hipStream_t)stream, D, N, sqnorm, X, d, nullptr,
                                     1.f, nullptr);
    else hipLaunchKernelGGL(tile_pair_kernel<0>, dim3(nt, nt), dim3(256), 0, (hipStream_t)stream, D, N, sqnorm, X, d, nullptr, 1.f, nullptr);
    return jamie_launch_status("jamie_gram_to_distances");
}

extern "C" int jamie_gram_to_scaled_sqdist(float* D, const float* sqnorm, const float* X, long long N, int d, float scale,
                                           const float* rownorm, void* stream) {
    JAMIE_ARG(D && sqnorm && X && rownorm && N > 0 && N <= (1 << 24) && d > 0, "null pointer / 0 < N <= 2^24 / d > 0");
    JAMIE_ARG(scale > 0.f && scale < __builtin_inff(), "scale must be positive and finite");
    const int nt = dist_tiles(N);
    hipLaunchKernelGGL(tile_pair_kernel<3>, dim3(nt, nt), dim3(256), 0, (hipStream_t)stream, D, N, sqnorm, X, d, nullptr, scale,
                       rownorm);
    return jamie_launch_status("jamie_gram_to_scaled_sqdist");
}

extern "C" int jamie_row_normalise(const void* X, int is_f64, long long N, int d, int centre, float* out, float* norm, void* stream) {
    JAMIE_ARG(X && out && norm && N > 0 && d > 0, "null pointer / empty");
    JAMIE_ARG((is_f64 == 0 || is_f64 == 1) && (centre == 0 || centre == 1), "is_f64 and centre are 0 or 1");
    const dim3 grid((unsigned)((N + 3) / 4));
    if (is_f64)
        hipLaunchKernelGGL(row_normalise_kernel<double>, grid, dim3(256), 0, (hipStream_t)stream, (const double*)X, N, d, centre, out, norm);
    else
        hipLaunchKernelGGL(row_normalise_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)X, N, d, centre, out, norm);
    return jamie_launch_status("jamie_row_normalise");
}

extern "C" int jamie_pairwise_absdiff(const float* X, long long N, int d, int op, float* D, void* stream) {
    JAMIE_ARG(X && D && N > 0 && N <= (1 << 24) && d > 0, "null pointer / 0 < N <= 2^24 / d > 0");
    JAMIE_ARG(op == 0 || op == 1, "op is 0 (sum) or 1 (max)");
    hipStream_t st = (hipStream_t)stream;
    const int vec = (d % 4 == 0) && ((uintptr_t)X & 15) == 0;
    const long long nt = (N + AD_T - 1) / AD_T;
    long long step = AD_LAUNCH_WORK / ((long long)AD_T * N * d);            // rows of tiles per launch
    step = step < 1 ? 1 : (step > 65535 ? 65535 : step);
    for (long long t0 = 0; t0 < nt; t0 += step) {
        const long long n = nt - t0 < step ? nt - t0 : step;
        if (op == 0) hipLaunchKernelGGL(absdiff_kernel<0>, dim3((unsigned)nt, (unsigned)n), dim3(256), 0, st, X, N, d, vec, t0, D);
        else hipLaunchKernelGGL(absdiff_kernel<1>, dim3((unsigned)nt, (unsigned)n), dim3(256), 0, st, X, N, d, vec, t0, D);
    }
    return jamie_launch_status("jamie_pairwise_absdiff");
}

extern "C" int jamie_knn_topk(const float* D, long long N, int K, int32_t* idx, void* stream) {
    JAMIE_ARG(D && idx && N > 0 && N <= (1 << 24), "null pointer / 0 < N <= 2^24");
    JAMIE_ARG(K >= 1 && K <= N && K <= TOPK_MAX, "1 <= K <= min(N, 1024)");
    hipLaunchKernelGGL(topk_kernel, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, D, N, K, idx);
    return jamie_launch_status("jamie_knn_topk");
}

extern "C" int jamie_knn_weights(const float* X, long long N, int d, const int32_t* idx, int K, float* w, void* stream) {
    JAMIE_ARG(X && idx && w && N > 0 && d > 0 && K >= 1, "null pointer / empty");
    hipLaunchKernelGGL(knn_weight_kernel, dim3((unsigned)((N * K + 3) / 4)), dim3(256), 0, (hipStream_t)stream, X, N, d, idx, K, w);
    return jamie_launch_status("jamie_knn_weights");
}

extern "C" int jamie_knn_graph_init(float* D, long long N, const int32_t* idx, const float* w, int K, int k, void* stream) {
    JAMIE_ARG(D && idx && w && N > 0 && K >= 1 && k >= 1 && k <= K, "null pointer / 1 <= k <= K");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(graph_fill_kernel, dim3((unsigned)N), dim3(256), 0, st, D, N);
    hipLaunchKernelGGL(graph_scatter_kernel, dim3((unsigned)((N * k + 255) / 256)), dim3(256), 0, st, D, N, idx, w, K, k);
    return jamie_launch_status("jamie_knn_graph_init");
}

extern "C" int jamie_apsp_fw(float* D, long long N, void* stream) {
    JAMIE_ARG(D && N > 0 && N <= (1 << 24), "null pointer / 0 < N <= 2^24");
    hipStream_t st = (hipStream_t)stream;
    const int nb = (int)((N + FW_T - 1) / FW_T);
    for (int r = 0; r < nb; ++r) {
        hipLaunchKernelGGL(fw_phase12_kernel<0>, dim3(1), dim3(1024), 0, st, D, N, r);
        if (nb > 1) {
            hipLaunchKernelGGL(fw_phase12_kernel<1>, dim3(nb), dim3(1024), 0, st, D, N, r);
            hipLaunchKernelGGL(fw_phase12_kernel<2>, dim3(nb), dim3(1024), 0, st, D, N, r);
            hipLaunchKernelGGL(fw_phase3_kernel, dim3(nb, nb), dim3(256), 0, st, D, N, r);
        }
        const int rc = jamie_launch_status("jamie_apsp_fw");
        if (rc) return rc;
    }
    return 0;
}

extern "C" int jamie_apsp_finalise(float* D, long long N, float* partials, long long n_partials, float* maxv, void* stream) {
    JAMIE_ARG(D && partials && maxv && N > 0 && N <= (1 << 24), "null pointer / 0 < N <= 2^24");
    const int nt = dist_tiles(N);
    JAMIE_ARG(n_partials >= (long long)nt * nt, "n_partials < jamie_dist_workspace(N)");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(tile_pair_kernel<2>, dim3(nt, nt), dim3(256), 0, st, D, N, nullptr, nullptr, 0, partials, 1.f, nullptr);
    hipLaunchKernelGGL(max_reduce_kernel, dim3(1), dim3(256), 0, st, partials, (long long)nt * nt, maxv);
    const long long blocks = (N * N + 255) / 256;
    hipLaunchKernelGGL(fill_unreachable_kernel, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, st, D, N * N, maxv);
    return jamie_launch_status("jamie_apsp_finalise");
}

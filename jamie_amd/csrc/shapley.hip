// Shapley attributions on the device (include/jamie_hip.h "Shapley attributions on the device"; jamie_amd/shapley.py): the permutation-
// sampling estimator of the Shapley value of input features ("players") for the values imputed for another modality.
//
// Walk (jamie_shapley_walk_rows).  An order is walked as removals: step m sets player f_m of every cell to its background.  The first
// encoder layer is linear, so a step changes a cell's pre-activation by one rank-one term,
//     s_0 = state,   s_m = fmaf(-(x[c, f_m] - bg[f_m]), W0[:, f_m], s_{m-1}),   out[m n + c, :] = lrelu(bn(s_m[c, :]))   (m = 0 .. g),
// with the BatchNorm-eval + LeakyReLU expression of the GEMM's EPI_BN_EVAL epilogue, and on return state = s_g: the next segment of
// the same order continues from it.  The kernel is bound by its (g + 1) n h stores.  A lane owns four consecutive hidden units
// (16-byte loads and stores) of WALK_CELLS cells, a wave 256 hidden units, a workgroup 4 x WALK_CELLS cells.  The g columns of W0 are
// gathered once per launch into a transposed scratch WT [g, h4] in walk order; a lane reads WALK_G rows of it ahead of the chain
// (they do not depend on it), uses each for its WALK_CELLS cells -- independent fmaf chains -- and the factor x - bg is a
// wave-uniform load.  No LDS, no atomics, no scratch memory.  `feat` is validated on the host before anything is launched.
//
// Accumulation (jamie_shapley_accumulate).  phi[c, pos[m], j] += (double)Y[m n + c, tcol[j]] - (double)Y[(m + 1) n + c, tcol[j]].
// A thread owns one (cell, target) pair of ACC_STEPS consecutive steps and keeps the previous row's value; `pos` is distinct within a
// launch, so every element of phi has one owner: no reduction, no atomics.  Threads run along j.
//
// Summary (jamie_shapley_summarise).  sum_abs[e] += sum_c |phi[c, e]|, sum[e] += sum_c phi[c, e]: a thread adds the SUM_ROWS cells of a
// row block in order into an fp64 partial, the finishing kernel adds an element's partials in order and the total onto the outputs.
#include <vector>

#include "common.h"

namespace {

constexpr int WALK_G = 8;              // rows of WT a lane holds ahead of the chain (jamie_amd/shapley.py GROUP)
constexpr int WALK_CELLS = 4;          // cells of a lane: independent chains that share the rows of WT
constexpr int WALK_COLS = 256;         // hidden units of a workgroup: 64 lanes x 4
constexpr int WALK_ROWS = 4 * WALK_CELLS;   // cells of a workgroup: 4 waves x WALK_CELLS
constexpr int ACC_STEPS = 8;           // steps of a thread of the accumulation
constexpr int SUM_ROWS = 512;          // cells per fp64 partial (jamie_amd/_native.py SHAPLEY_ROWS)

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// WT[k, m] = W0[m, feat[k]] for m < h, 0 for h <= m < h4
__global__ __launch_bounds__(256) void shapley_stage_kernel(const float* __restrict__ W0, long long ldw, const int* __restrict__ feat,
                                                            int h, int h4, float* __restrict__ WT) {
    const int m = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
    if (m >= h4) return;
    WT[(long long)k * h4 + m] = m < h ? W0[(long long)m * ldw + feat[k]] : 0.f;
}

// columns [col, col + 4) of a row; 0 where the column does not exist
__device__ __forceinline__ float4 load4(const float* __restrict__ p, int col, int n, bool vec) {
    if (vec) return *reinterpret_cast<const float4*>(p);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    v.x = p[0];
    if (col + 1 < n) v.y = p[1];
    if (col + 2 < n) v.z = p[2];
    if (col + 3 < n) v.w = p[3];
    return v;
}

__device__ __forceinline__ void store4(float* __restrict__ p, int col, int n, bool vec, const float4& v) {
    if (vec) {
        *reinterpret_cast<float4*>(p) = v;
        return;
    }
    p[0] = v.x;
    if (col + 1 < n) p[1] = v.y;
    if (col + 2 < n) p[2] = v.z;
    if (col + 3 < n) p[3] = v.w;
}

// eval BatchNorm + LeakyReLU in the operation order of the GEMM's EPI_BN_EVAL epilogue (gemm_f32.hip; csrc/impact.hip bn_lrelu)
__device__ __forceinline__ float bn_lrelu(float v, float mean, float scale, float shift, float slope) {
    const float y = (v - mean) * scale + shift;
    return y > 0.f ? y : slope * y;
}

__device__ __forceinline__ float4 bn_lrelu4(const float4& s, const float4& mu, const float4& sc, const float4& sh, float slope) {
    return make_float4(bn_lrelu(s.x, mu.x, sc.x, sh.x, slope), bn_lrelu(s.y, mu.y, sc.y, sh.y, slope),
                       bn_lrelu(s.z, mu.z, sc.z, sh.z, slope), bn_lrelu(s.w, mu.w, sc.w, sh.w, slope));
}

template <bool VEC>
__global__ __launch_bounds__(256) void shapley_walk_kernel(float* __restrict__ state, long long lds, const float* __restrict__ X,
                                                           long long ldx, const float* __restrict__ bg, const float* __restrict__ WT,
                                                           int h4, const int* __restrict__ feat, int n, int h, int g,
                                                           const float* __restrict__ rmean, const float* __restrict__ rvar,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                           float slope, float* __restrict__ out, long long ldo) {
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);        // (the same in every lane of a wave)
    const int col = blockIdx.x * WALK_COLS + lane * 4;
    const int c0 = blockIdx.y * WALK_ROWS + w * WALK_CELLS;
    if (col >= h || c0 >= n) return;
    const bool vec = VEC;                                          // (VEC: h, every leading dimension and pointer in units of 16 bytes)
    const float4 mu = load4(rmean + col, col, h, vec), var = load4(rvar + col, col, h, vec);
    const float4 ga = load4(gamma + col, col, h, vec), sh = load4(beta + col, col, h, vec);
    const float4 sc = make_float4(rsqrtf(var.x + eps) * ga.x, rsqrtf(var.y + eps) * ga.y, rsqrtf(var.z + eps) * ga.z,
                                  rsqrtf(var.w + eps) * ga.w);
    const int nc = n - c0 < WALK_CELLS ? n - c0 : WALK_CELLS;      // cells of this wave: 1 .. WALK_CELLS (wave-uniform)
    float4 s[WALK_CELLS];
#pragma unroll
    for (int r = 0; r < WALK_CELLS; ++r) {
        const int c = c0 + (r < nc ? r : 0);                       // (a cell that does not exist repeats the first and stores nothing)
        s[r] = load4(state + (long long)c * lds + col, col, h, vec);
        if (r < nc) store4(out + (long long)c * ldo + col, col, h, vec, bn_lrelu4(s[r], mu, sc, sh, slope));
    }
    for (int m0 = 0; m0 < g; m0 += WALK_G) {
        float4 wk[WALK_G];
        float dl[WALK_CELLS][WALK_G];
#pragma unroll
        for (int k = 0; k < WALK_G; ++k) {                         // every load of the block ahead of the chain; past the end: the last step
            const int m = m0 + k < g ? m0 + k : g - 1;
            wk[k] = *reinterpret_cast<const float4*>(WT + (long long)m * h4 + col);
            const int f = feat[m];
            const float b = bg[f];
#pragma unroll
            for (int r = 0; r < WALK_CELLS; ++r) dl[r][k] = X[(long long)(c0 + (r < nc ? r : 0)) * ldx + f] - b;
        }
#pragma unroll
        for (int k = 0; k < WALK_G; ++k) {
            if (m0 + k < g) {
#pragma unroll
                for (int r = 0; r < WALK_CELLS; ++r) {
                    s[r].x = fmaf(-dl[r][k], wk[k].x, s[r].x);
                    s[r].y = fmaf(-dl[r][k], wk[k].y, s[r].y);
                    s[r].z = fmaf(-dl[r][k], wk[k].z, s[r].z);
                    s[r].w = fmaf(-dl[r][k], wk[k].w, s[r].w);
                    if (r < nc)
                        store4(out + ((long long)(m0 + k + 1) * n + c0 + r) * ldo + col, col, h, vec, bn_lrelu4(s[r], mu, sc, sh, slope));
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < WALK_CELLS; ++r)
        if (r < nc) store4(state + (long long)(c0 + r) * lds + col, col, h, vec, s[r]);
}

// thread (c, j) of the steps [blockIdx.y * ACC_STEPS, + ACC_STEPS): phi[c, pos[m], j] += Y[m n + c, tj] - Y[(m + 1) n + c, tj]
__global__ __launch_bounds__(256) void shapley_accumulate_kernel(const float* __restrict__ Y, long long ldy, int n, int g,
                                                                 const int* __restrict__ pos, int F, const int* __restrict__ tcol, int T,
                                                                 double* __restrict__ phi) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)n * T) return;
    const int c = (int)(idx / T), j = (int)(idx - (long long)c * T);
    const int tj = tcol ? tcol[j] : j;
    const int m0 = blockIdx.y * ACC_STEPS;
    const int m1 = m0 + ACC_STEPS < g ? m0 + ACC_STEPS : g;
    const float* __restrict__ y = Y + (long long)c * ldy + tj;
    double* __restrict__ ph = phi + (long long)c * F * T + j;
    const long long step = (long long)n * ldy;
    double a = (double)y[(long long)m0 * step];
    for (int m = m0; m < m1; ++m) {
        const double b = (double)y[(long long)(m + 1) * step];
        double* __restrict__ q = ph + (long long)pos[m] * T;
        *q += a - b;
        a = b;
    }
}

// part[rb, 0, e] = sum over the cells of row block rb of |phi[c, e]|, part[rb, 1, e] = the same of phi[c, e]: in order
__global__ __launch_bounds__(256) void shapley_partial_kernel(const double* __restrict__ phi, int n, long long elems,
                                                              double* __restrict__ part) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= elems) return;
    const int r0 = blockIdx.y * SUM_ROWS;
    const int r1 = r0 + SUM_ROWS < n ? r0 + SUM_ROWS : n;
    const double* __restrict__ p = phi + (long long)r0 * elems + e;
    double sa = 0.0, ss = 0.0;
    int c = r0;
    for (; c + 3 < r1; c += 4, p += 4 * elems) {
        const double v0 = p[0], v1 = p[elems], v2 = p[2 * elems], v3 = p[3 * elems];
        sa += fabs(v0);
        ss += v0;
        sa += fabs(v1);
        ss += v1;
        sa += fabs(v2);
        ss += v2;
        sa += fabs(v3);
        ss += v3;
    }
    for (; c < r1; ++c, p += elems) {
        const double v = p[0];
        sa += fabs(v);
        ss += v;
    }
    part[(long long)blockIdx.y * 2 * elems + e] = sa;
    part[((long long)blockIdx.y * 2 + 1) * elems + e] = ss;
}

// sum_abs[e] += the partials of element e in row-block order; sum[e] likewise
__global__ __launch_bounds__(256) void shapley_finish_kernel(const double* __restrict__ part, long long elems, int nrb,
                                                             double* __restrict__ sum_abs, double* __restrict__ sum) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= elems) return;
    double sa = 0.0, ss = 0.0;
    for (int rb = 0; rb < nrb; ++rb) {
        sa += part[(long long)rb * 2 * elems + e];
        ss += part[((long long)rb * 2 + 1) * elems + e];
    }
    sum_abs[e] += sa;
    sum[e] += ss;
}

// every entry in [0, bound) and no entry twice
bool distinct_in_range(const int32_t* v, int count, int bound) {
    std::vector<unsigned char> seen((size_t)bound, 0);
    for (int k = 0; k < count; ++k) {
        if (v[k] < 0 || v[k] >= bound || seen[(size_t)v[k]]) return false;
        seen[(size_t)v[k]] = 1;
    }
    return true;
}

}  // namespace

extern "C" int jamie_shapley_walk_rows(float* state, long long lds, const float* X, long long ldx, const float* bg, const float* W0,
                                       long long ldw, const int32_t* feat, const int32_t* feat_host, int n, int h, int d, int g,
                                       const float* running_mean, const float* running_var, const float* gamma, const float* beta,
                                       float eps, float slope, float* out, long long ldo, void* ws, long long ws_bytes, void* stream) {
    JAMIE_ARG(n > 0 && h > 0 && g > 0 && d > 0, "n, h, d and g must be positive");
    JAMIE_ARG(state && X && bg && W0 && feat && feat_host && running_mean && running_var && gamma && beta && out && ws, "null pointer");
    JAMIE_ARG(lds >= h && ldx >= d && ldw >= d && ldo >= h, "lds < h, ldx < d, ldw < d or ldo < h");
    JAMIE_ARG(((long long)g + 1) * n < 2147483647ll, "(g + 1) * n < 2^31");
    for (int k = 0; k < g; ++k) JAMIE_ARG(feat_host[k] >= 0 && feat_host[k] < d, "a feature index outside [0, d)");
    const int h4 = (h + 3) / 4 * 4;
    JAMIE_ARG(ws_bytes >= (long long)g * h4 * 4 && aligned16(ws), "workspace: 4 g ceil4(h) bytes on a 16-byte boundary");
    const unsigned ct = (unsigned)((h + WALK_COLS - 1) / WALK_COLS), rb = (unsigned)((n + WALK_ROWS - 1) / WALK_ROWS);
    JAMIE_ARG(rb <= 65535 && g <= 65535, "n <= 65535 * 16, g <= 65535");
    hipStream_t st = (hipStream_t)stream;
    float* WT = (float*)ws;
    hipLaunchKernelGGL(shapley_stage_kernel, dim3((unsigned)((h4 + 255) / 256), (unsigned)g), dim3(256), 0, st, W0, ldw, feat, h, h4, WT);
    const bool vec = h % 4 == 0 && lds % 4 == 0 && ldo % 4 == 0 && aligned16(state) && aligned16(out) && aligned16(running_mean) &&
                     aligned16(running_var) && aligned16(gamma) && aligned16(beta);
    if (vec)
        hipLaunchKernelGGL((shapley_walk_kernel<true>), dim3(ct, rb), dim3(256), 0, st, state, lds, X, ldx, bg, WT, h4, feat, n, h, g,
                           running_mean, running_var, gamma, beta, eps, slope, out, ldo);
    else
        hipLaunchKernelGGL((shapley_walk_kernel<false>), dim3(ct, rb), dim3(256), 0, st, state, lds, X, ldx, bg, WT, h4, feat, n, h, g,
                           running_mean, running_var, gamma, beta, eps, slope, out, ldo);
    return jamie_launch_status("jamie_shapley_walk_rows");
}

extern "C" int jamie_shapley_accumulate(const float* Y, long long ldy, int n, int dt, int g, const int32_t* pos, const int32_t* pos_host,
                                        int F, const int32_t* tcol, const int32_t* tcol_host, int T, double* phi, void* stream) {
    JAMIE_ARG(n > 0 && dt > 0 && g > 0 && F > 0 && T > 0, "n, dt, g, F and T must be positive");
    JAMIE_ARG(Y && pos && pos_host && phi, "null pointer");
    JAMIE_ARG((tcol == nullptr) == (tcol_host == nullptr), "tcol and tcol_host: both or neither");
    JAMIE_ARG(ldy >= dt && T <= dt && g <= F, "ldy < dt, T > dt or g > F");
    JAMIE_ARG(tcol != nullptr || T == dt, "without tcol, T must be dt");
    JAMIE_ARG(((long long)g + 1) * n < 2147483647ll, "(g + 1) * n < 2^31");
    JAMIE_ARG(distinct_in_range(pos_host, g, F), "pos: distinct positions in [0, F)");
    if (tcol_host) JAMIE_ARG(distinct_in_range(tcol_host, T, dt), "tcol: distinct columns in [0, dt)");
    const long long blocks = ((long long)n * T + 255) / 256;
    const int chunks = (g + ACC_STEPS - 1) / ACC_STEPS;
    JAMIE_ARG(blocks < 2147483647ll && chunks <= 65535, "n * T < 2^39, g <= 65535 * 8");
    hipLaunchKernelGGL(shapley_accumulate_kernel, dim3((unsigned)blocks, (unsigned)chunks), dim3(256), 0, (hipStream_t)stream, Y, ldy, n, g,
                       pos, F, tcol, T, phi);
    return jamie_launch_status("jamie_shapley_accumulate");
}

extern "C" int jamie_shapley_summarise(const double* phi, int n, long long elems, double* sum_abs, double* sum, void* ws,
                                       long long ws_bytes, void* stream) {
    JAMIE_ARG(n > 0 && elems > 0, "n and elems must be positive");
    JAMIE_ARG(phi && sum_abs && sum && ws, "null pointer");
    const int nrb = (n + SUM_ROWS - 1) / SUM_ROWS;
    const long long blocks = (elems + 255) / 256;
    JAMIE_ARG(nrb <= 65535 && blocks < 2147483647ll, "n <= 65535 * 512, elems < 2^39");
    JAMIE_ARG(ws_bytes >= 16 * elems * nrb && ((uintptr_t)ws & 7) == 0, "workspace: 16 elems ceil(n / 512) bytes on an 8-byte boundary");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(shapley_partial_kernel, dim3((unsigned)blocks, (unsigned)nrb), dim3(256), 0, st, phi, n, elems, (double*)ws);
    hipLaunchKernelGGL(shapley_finish_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const double*)ws, elems, nrb, sum_abs, sum);
    return jamie_launch_status("jamie_shapley_summarise");
}

// Feature impact on the device (include/jamie_hip.h "Feature impact on the device"; jamie_amd/impact.py): what the imputed values of
// one modality lose when one input feature of the other is replaced by a background value.
//
// Occlusion (jamie_occlusion_rows).  The first encoder layer is linear, so replacing feature f of a cell changes its pre-activation
// H = W0 x + b by the rank-one term (bg_f - x_f) W0[:, f]: the d -> 2d product is taken once per cell chunk and this kernel writes
// the first hidden activation of every (feature, cell) pair from it,
//     out[k n + c, m] = lrelu(bn(H[c, m] + (bg[feat[k]] - X[c, feat[k]]) W0[m, feat[k]])),
// with the BatchNorm-eval + LeakyReLU expression of the GEMM's EPI_BN_EVAL epilogue.  It is bound by its g n h stores: a lane owns
// four consecutive columns m (16-byte loads and stores), a workgroup a tile of 256 columns x OCC_ROWS cells x OCC_G features.  The g
// columns of W0 are gathered once per launch into a transposed scratch WT [g, h4] (the column reads are strided; everything the main
// kernel reads is contiguous), a lane keeps its four columns of the OCC_G features in registers, and a row of H is read once per
// feature group, not once per feature.  `feat` is validated on the host before anything is launched.
//
// Accumulation (jamie_impact_accumulate).  acc[k, j] += sum_c (Y[k n + c, j] - R[c, j])^2 with the difference and the square in
// fp64.  A workgroup owns 64 columns x ACC_ROWS cells of one feature (16 lanes x float4 across the columns, 16 row groups, 4 rows
// of both matrices in flight per thread), adds its 16 row groups in order and writes an fp64 partial; the finishing kernel deals
// the row blocks of an element to 32 slices (slice s adds blocks s, s + 32, ... in order), adds the slices in order and adds the
// total onto acc, one thread per element.  No atomics: every bit is the same from run to run.
#include "common.h"

namespace {

constexpr int OCC_G = 8;               // features of a group: a lane holds 4 columns of W0 for each (jamie_amd/impact.py GROUP)
constexpr int OCC_COLS = 256;          // columns of a workgroup: 64 lanes x 4
constexpr int OCC_ROWS = 32;           // cells of a workgroup: 4 waves x 8
constexpr int ACC_ROWS = 512;          // cells per fp64 partial (jamie_amd/impact.py ROW_BLOCK)
constexpr int ACC_RG = 16;             // row groups of an accumulating workgroup
constexpr int FIN_F = 8, FIN_S = 32;   // the finishing kernel: elements and slices per workgroup

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// WT[k, m] = W0[m, feat[k]] for m < h, 0 for h <= m < h4
__global__ __launch_bounds__(256) void occlusion_stage_kernel(const float* __restrict__ W0, long long ldw, const int* __restrict__ feat,
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

// eval BatchNorm + LeakyReLU in the operation order of the GEMM's EPI_BN_EVAL epilogue (gemm_f32.hip)
__device__ __forceinline__ float bn_lrelu(float v, float mean, float scale, float shift, float slope) {
    const float y = (v - mean) * scale + shift;
    return y > 0.f ? y : slope * y;
}

template <bool VEC>
__global__ __launch_bounds__(256) void occlusion_rows_kernel(const float* __restrict__ H, long long ldh, const float* __restrict__ X,
                                                             long long ldx, const float* __restrict__ bg, const float* __restrict__ WT,
                                                             int h4, const int* __restrict__ feat, int n, int h, int g,
                                                             const float* __restrict__ rmean, const float* __restrict__ rvar,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                             float slope, float* __restrict__ out, long long ldo) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int col = blockIdx.x * OCC_COLS + lane * 4;
    if (col >= h) return;
    const bool vec = VEC;                                          // (VEC: h, every leading dimension and pointer in units of 16 bytes)
    const int k0 = blockIdx.z * OCC_G;
    const int gk = g - k0 < OCC_G ? g - k0 : OCC_G;                // (the same in every thread)
    const float4 mu = load4(rmean + col, col, h, vec), var = load4(rvar + col, col, h, vec);
    const float4 ga = load4(gamma + col, col, h, vec), sh = load4(beta + col, col, h, vec);
    const float4 sc = make_float4(rsqrtf(var.x + eps) * ga.x, rsqrtf(var.y + eps) * ga.y, rsqrtf(var.z + eps) * ga.z,
                                  rsqrtf(var.w + eps) * ga.w);
    float4 wk[OCC_G];
    int fk[OCC_G];
    float bk[OCC_G];
#pragma unroll
    for (int k = 0; k < OCC_G; ++k) {
        const bool on = k < gk;
        wk[k] = on ? *reinterpret_cast<const float4*>(WT + (long long)(k0 + k) * h4 + col) : make_float4(0.f, 0.f, 0.f, 0.f);
        fk[k] = on ? feat[k0 + k] : 0;
        bk[k] = on ? bg[fk[k]] : 0.f;
    }
    const int r0 = blockIdx.y * OCC_ROWS;
    const int r1 = r0 + OCC_ROWS < n ? r0 + OCC_ROWS : n;
    for (int c = r0 + w; c < r1; c += 4) {
        const float4 hv = load4(H + (long long)c * ldh + col, col, h, vec);
        const float* __restrict__ xr = X + (long long)c * ldx;
#pragma unroll
        for (int k = 0; k < OCC_G; ++k) {
            if (k < gk) {
                const float dl = bk[k] - xr[fk[k]];
                float4 o;
                o.x = bn_lrelu(fmaf(dl, wk[k].x, hv.x), mu.x, sc.x, sh.x, slope);
                o.y = bn_lrelu(fmaf(dl, wk[k].y, hv.y), mu.y, sc.y, sh.y, slope);
                o.z = bn_lrelu(fmaf(dl, wk[k].z, hv.z), mu.z, sc.z, sh.z, slope);
                o.w = bn_lrelu(fmaf(dl, wk[k].w, hv.w), mu.w, sc.w, sh.w, slope);
                store4(out + ((long long)(k0 + k) * n + c) * ldo + col, col, h, vec, o);
            }
        }
    }
}

__device__ __forceinline__ void sq_add(double (&acc)[4], const float4& y, const float4& r) {
    const float ys[4] = {y.x, y.y, y.z, y.w}, rs[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const double e = (double)ys[q] - (double)rs[q];
        acc[q] += e * e;
    }
}

// part[(rb * g + k) * dt + j]: the sum over the cells of row block rb
__global__ __launch_bounds__(256) void impact_partial_kernel(const float* __restrict__ Y, long long ldy, const float* __restrict__ R,
                                                             long long ldr, int n, int dt, int g, int vec, double* __restrict__ part) {
    __shared__ double sm[ACC_RG][64];
    const int c4 = threadIdx.x & 15, rg = threadIdx.x >> 4;
    const int col = blockIdx.x * 64 + c4 * 4, k = blockIdx.z;
    const int r0 = blockIdx.y * ACC_ROWS;
    const int r1 = r0 + ACC_ROWS < n ? r0 + ACC_ROWS : n;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    if (col < dt) {
        const bool v = vec != 0 && col + 3 < dt;
        const float* __restrict__ Yk = Y + (long long)k * n * ldy + col;
        const float* __restrict__ Rc = R + col;
        int c = r0 + rg;
        for (; c + 3 * ACC_RG < r1; c += 4 * ACC_RG) {
            float4 y[4], r[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                y[u] = load4(Yk + (long long)(c + ACC_RG * u) * ldy, col, dt, v);
                r[u] = load4(Rc + (long long)(c + ACC_RG * u) * ldr, col, dt, v);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) sq_add(acc, y[u], r[u]);
        }
        for (; c < r1; c += ACC_RG) sq_add(acc, load4(Yk + (long long)c * ldy, col, dt, v), load4(Rc + (long long)c * ldr, col, dt, v));
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) sm[rg][c4 * 4 + q] = acc[q];
    __syncthreads();
    if (threadIdx.x < 64) {
        const int oc = blockIdx.x * 64 + threadIdx.x;
        if (oc < dt) {
            double t = 0.0;
            for (int i = 0; i < ACC_RG; ++i) t += sm[i][threadIdx.x];
            part[((long long)blockIdx.y * g + k) * dt + oc] = t;
        }
    }
}

// acc[e] += the partials of element e = k * dt + j: 32 slices of row blocks, each added in order, then the slices in order
__global__ __launch_bounds__(256) void impact_finish_kernel(const double* __restrict__ part, long long elems, int nrb,
                                                            double* __restrict__ acc) {
    __shared__ double sm[FIN_S][FIN_F];
    const int c = threadIdx.x % FIN_F, sl = threadIdx.x / FIN_F;
    const long long e = (long long)blockIdx.x * FIN_F + c;
    double s = 0.0;
    if (e < elems)
        for (int rb = sl; rb < nrb; rb += FIN_S) s += part[(long long)rb * elems + e];
    sm[sl][c] = s;
    __syncthreads();
    if (sl != 0 || e >= elems) return;
    double t = 0.0;
    for (int i = 0; i < FIN_S; ++i) t += sm[i][c];
    acc[e] += t;
}

}  // namespace

extern "C" int jamie_occlusion_rows(const float* H, long long ldh, const float* X, long long ldx, const float* bg, const float* W0,
                                    long long ldw, const int32_t* feat, const int32_t* feat_host, int n, int h, int d, int g,
                                    const float* running_mean, const float* running_var, const float* gamma, const float* beta,
                                    float eps, float slope, float* out, long long ldo, void* ws, long long ws_bytes, void* stream) {
    JAMIE_ARG(n > 0 && h > 0 && g > 0 && d > 0, "n, h, d and g must be positive");
    JAMIE_ARG(H && X && bg && W0 && feat && feat_host && running_mean && running_var && gamma && beta && out && ws, "null pointer");
    JAMIE_ARG(ldh >= h && ldx >= d && ldw >= d && ldo >= h, "ldh < h, ldx < d, ldw < d or ldo < h");
    JAMIE_ARG((long long)g * n < 2147483647ll, "g * n < 2^31");
    for (int k = 0; k < g; ++k) JAMIE_ARG(feat_host[k] >= 0 && feat_host[k] < d, "a feature index outside [0, d)");
    const int h4 = (h + 3) / 4 * 4;
    JAMIE_ARG(ws_bytes >= (long long)g * h4 * 4 && aligned16(ws), "workspace: 4 g ceil4(h) bytes on a 16-byte boundary");
    const unsigned ct = (unsigned)((h + OCC_COLS - 1) / OCC_COLS), rb = (unsigned)((n + OCC_ROWS - 1) / OCC_ROWS);
    const unsigned gz = (unsigned)((g + OCC_G - 1) / OCC_G);
    JAMIE_ARG(rb <= 65535 && gz <= 65535 && g <= 65535, "n <= 65535 * 32, g <= 65535");
    hipStream_t st = (hipStream_t)stream;
    float* WT = (float*)ws;
    hipLaunchKernelGGL(occlusion_stage_kernel, dim3((unsigned)((h4 + 255) / 256), (unsigned)g), dim3(256), 0, st, W0, ldw, feat, h, h4, WT);
    const bool vec = h % 4 == 0 && ldh % 4 == 0 && ldo % 4 == 0 && aligned16(H) && aligned16(out) && aligned16(running_mean) &&
                     aligned16(running_var) && aligned16(gamma) && aligned16(beta);
    if (vec)
        hipLaunchKernelGGL((occlusion_rows_kernel<true>), dim3(ct, rb, gz), dim3(256), 0, st, H, ldh, X, ldx, bg, WT, h4, feat, n, h, g,
                           running_mean, running_var, gamma, beta, eps, slope, out, ldo);
    else
        hipLaunchKernelGGL((occlusion_rows_kernel<false>), dim3(ct, rb, gz), dim3(256), 0, st, H, ldh, X, ldx, bg, WT, h4, feat, n, h, g,
                           running_mean, running_var, gamma, beta, eps, slope, out, ldo);
    return jamie_launch_status("jamie_occlusion_rows");
}

extern "C" int jamie_impact_accumulate(const float* Y, long long ldy, const float* R, long long ldr, int n, int dt, int g, double* acc,
                                       void* ws, long long ws_bytes, void* stream) {
    JAMIE_ARG(n > 0 && dt > 0 && g > 0, "n, dt and g must be positive");
    JAMIE_ARG(Y && R && acc && ws, "null pointer");
    JAMIE_ARG(ldy >= dt && ldr >= dt, "ldy < dt or ldr < dt");
    JAMIE_ARG((long long)g * n < 2147483647ll, "g * n < 2^31");
    const int nrb = (n + ACC_ROWS - 1) / ACC_ROWS;
    JAMIE_ARG(nrb <= 65535 && g <= 65535, "n <= 65535 * 512, g <= 65535");
    const long long elems = (long long)g * dt;
    JAMIE_ARG(ws_bytes >= 8 * elems * nrb && ((uintptr_t)ws & 7) == 0, "workspace: 8 g dt ceil(n / 512) bytes on an 8-byte boundary");
    JAMIE_ARG((elems + FIN_F - 1) / FIN_F < 2147483647ll, "g * dt < 2^34");
    hipStream_t st = (hipStream_t)stream;
    const int vec = ldy % 4 == 0 && ldr % 4 == 0 && aligned16(Y) && aligned16(R);
    hipLaunchKernelGGL(impact_partial_kernel, dim3((unsigned)((dt + 63) / 64), (unsigned)nrb, (unsigned)g), dim3(256), 0, st, Y, ldy, R, ldr,
                       n, dt, g, vec, (double*)ws);
    hipLaunchKernelGGL(impact_finish_kernel, dim3((unsigned)((elems + FIN_F - 1) / FIN_F)), dim3(256), 0, st, (const double*)ws, elems, nrb,
                       acc);
    return jamie_launch_status("jamie_impact_accumulate");
}

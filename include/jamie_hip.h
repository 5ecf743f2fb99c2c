/* jamie_hip.h — C ABI of libjamie_hip.so: the MI355X (gfx950) kernels behind JAMIE's coupled-VAE
 * training / inference hot path.
 *
 * The reference (Oafish1/JAMIE v4.4.5) is pure Python on PyTorch ATen CPU kernels and has no FFI of its
 * own; its seam for this path is the duck-typed `model_class=` protocol (jamie/jamie.py:47,71,472-479,611)
 * plus the per-step ATen ops listed in SURVEY.md §2.1 (K1..K15).  Each entry point below replaces one
 * group of those ATen dispatches; the citation names the reference call site(s) it stands in for.
 * INTEGRATION.md shows the ctypes binding a JAMIE maintainer would add.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is DEVICE memory unless marked host;
 *   - the caller (PyTorch) owns all buffers; no entry point allocates, frees or synchronises;
 *   - every launch goes to the `stream` argument (a hipStream_t passed as void*), so calls are
 *     capturable into a hipGraph;
 *   - return value: 0 on success, <0 for an argument error, >0 a hipError_t; the message is available
 *     from jamie_last_error() (thread-local);
 *   - matrices are row-major fp32 with explicit leading dimensions (elements);
 *   - `rng` = device uint64[4] {seed, step, reserved, reserved}: counter-based Philox4x32-10 streams are
 *     derived from (seed, step, stream id, element index), so forward and backward regenerate identical
 *     dropout masks without storing them.  Tests pass explicit masks / noise instead.
 */
#ifndef JAMIE_HIP_H
#define JAMIE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JAMIE_MAX_GROUP 4      /* problems per grouped launch (modalities) */
#define JAMIE_MAX_GEMM_GROUP 8 /* problems per grouped GEMM launch (modalities x {dX, dW} + a skinny layer's dW riding along) */
#define JAMIE_MAX_GEMM_GROUP_F32 12 /* ... of jamie_gemm_f32 / _cfg (fp32: the four large layers' dW of two modalities + the two skinny layers' in one launch) */

const char* jamie_last_error(void);
int jamie_version(void);
/* number of fp32 loss partial slots a GEMM epilogue / latent kernel may write (sizing helper) */
int jamie_max_partials(void);
/* number of sum-of-squares partials (dW tiles + range chunks) jamie_clip_adam* accepts */
int jamie_max_norm_partials(void);

/* ---------------------------------------------------------------------------------------------
 * GEMM (fp32 in, fp32 accumulate on v_mfma_f32_32x32x2_f32).  Replaces every nn.Linear forward
 * (`addmm`, model.py:151,161,180,185,192,197,207) and its two autograd backward products
 * (jamie.py:734).  C[M,N] = op(A)[M,K] * op(B)[K,N]:
 *   layout JAMIE_NT: A is [M,K] (lda), B is [N,K] (ldb)   -> y  = x  W^T      (forward)
 *   layout JAMIE_NN: A is [M,K] (lda), B is [K,N] (ldb)   -> dx = dy W        (input gradient)
 *   layout JAMIE_TN: A is [K,M] (lda), B is [K,N] (ldb)   -> dW = dy^T x      (weight gradient)
 * ------------------------------------------------------------------------------------------- */
enum { JAMIE_NT = 0, JAMIE_NN = 1, JAMIE_TN = 2 };

enum {
    JAMIE_EPI_STORE   = 0, /* C = acc (+ bias[n])                                  (+= if accumulate) */
    JAMIE_EPI_MSE     = 1, /* d = acc + bias[n] - X[m,n]; C = d * scale; partial[block] = sum d^2
                              (Rec loss + its gradient, jamie.py:637-641; aux0 = X, ld aux_ld)        */
    JAMIE_EPI_BN_EVAL = 2, /* eval-mode Linear+BatchNorm1d+LeakyReLU: y = (acc + bias - aux0[n]) *
                              rsqrt(aux1[n] + eps) * aux2[n] + aux3[n]; C = y > 0 ? y : slope*y
                              (aux0..3 = running_mean, running_var, gamma, beta)                       */
};

typedef struct {
    const float* A; const float* B; float* C;
    const float* bias;          /* [N] or NULL */
    const float* aux0; const float* aux1; const float* aux2; const float* aux3;
    float* partial;             /* per-tile fp32 partial sums, slot m_tile + tiles_m * n_tile: the MSE term (EPI_MSE), or -- jamie_gemm_bf16,
                                 * large-tile configurations, EPI_STORE with splitk == 1 -- the sum of squares of the stored tile
                                 * (the dW launches hand the gradient norm its partial sums); or NULL */
    const int32_t* a_rows;      /* optional row gather for A (NT/NN: A row m -> a_rows[m]) or NULL */
    int M, N, K;
    int lda, ldb, ldc, aux_ld;
    int splitk;                 /* >= 1; slab s is written at C + s * slab_stride (no bias unless s==0) */
    long long slab_stride;
    int epi; int accumulate;
    float scale; float slope; float eps;
    float pscale;               /* EPI_MSE: partial[block] = pscale * sum d^2 (e.g. w_rec / (B*d)) */
    int b_tr;                   /* jamie_gemm_bf16 only: B is stored [K, N] row-major (N contiguous, ldb >= N) -- the dX
                                 * product dy W reads the weights W [out, in] as they are (model.py Linear backward), no
                                 * transposed copy; any large-tile configuration whose tile has 128 columns (23, 24, 25, 29 - 34; the
                                 * engine's dX launches run on 29) */
    int a_tr;                   /* jamie_gemm_bf16 only, with b_tr: A is stored [K, M] row-major (lda >= M) -- dW = dy^T a
                                 * reads dy [B, out] and a [B, in] as the layers produced them, no transposed activation
                                 * copies; the 128 x 128 large-tile configurations (24, 25, 29, 30, 32, 33, 34; the engine's dW
                                 * launches run on 29) */
    int store_nt;               /* non-temporal output stores (large-tile jamie_gemm_bf16 configurations, jamie_gemm_f32): for
                                 * outputs that are next read much later, e.g. weight gradients (read by the optimiser after the
                                 * whole backward pass) */
    int c_bf16;                 /* jamie_gemm_bf16, large-tile configurations, EPI_STORE without accumulate / split-K: C points to
                                 * bf16 [M, ldc] and the fp32 accumulators are rounded once on the way out (`partial` still sums
                                 * the squares of the fp32 values).  The weight gradients of the bf16 compute mode: 2 instead of 4
                                 * bytes per parameter written here and read again by jamie_clip_adam_g16 */
    int c_panel;                /* jamie_gemm_bf16, large-tile configurations, fp32 EPI_STORE without accumulate: every slab of C is
                                 * written in PANELS of P = JAMIE_PANEL columns -- element (m, n) at ((n / P) * M + m) * P + n % P
                                 * of its slab, slab_stride >= ceil(N / P) * P * M, ldc ignored -- the layout the BatchNorm launches
                                 * read (`panel` below): the column strip a BatchNorm workgroup owns is then whole contiguous blocks of
                                 * M x 4 P bytes per slab instead of M segments 4 N bytes apart (round 5: the pre-activations of
                                 * model.py:151-154 etc. go GEMM -> BatchNorm -> BatchNorm backward in this layout) */
} jamie_gemm_problem;
#ifndef JAMIE_PANEL
#define JAMIE_PANEL 16           /* columns per panel (16 fp32 = 64 bytes per row): a power of two >= 4.  8-column panels with 8-column BatchNorm
                                  * strips (three 256-thread workgroups per CU: 24 instead of 32 columns on the busiest CU) were built and
                                  * measured in round 5: +28 us per step, and +3 us with 8-column panels under the 16 / 32-column strips
                                  * (profiles/r05_ab_panel8_cq2_rejected.log) */
#endif
/* the panel width this library was built with (the host side lays its buffers out for it) */
int jamie_panel_width(void);

/* One launch computing up to JAMIE_MAX_GEMM_GROUP independent problems (the modalities of one layer; dX and dW together). */
int jamie_gemm_f32(const jamie_gemm_problem* problems /*host*/, int count, int layout, void* stream);
/* Same with an explicit tile configuration (tuning / benchmarks); cfg < 0 = choose by shape.  Configurations 0-18 run on the fp32
 * matrix pipe (v_mfma_f32_32x32x2_f32).  Configurations 20 (128 x 128 tiles) and 21 (256 x 128) run the SAME fp32 problem on the bf16 matrix pipe: every fp32 element is cut
 * into three bf16 pieces (x = hi + mid + lo, exact) and a product is six v_mfma_f32_32x32x16_bf16 into an fp32 accumulator -- fp32
 * inputs, fp32 outputs, error at the level of an fp32 product's own rounding (dropped terms <= 2^-21, typically 2^-24 of |a||b|); non-finite inputs
 * give NaN.  Every layout and epilogue; problems whose operands are not 16-byte aligned with leading dimensions and extents that
 * are multiples of 4 take the fp32 pipe's configuration of the same tile (17 / 15) instead.  The engine's default for the large layers
 * in fp32 mode (reference: the `addmm` / `mm` dispatches of model.py:151-207 and their autograd). */
int jamie_gemm_f32_cfg(const jamie_gemm_problem* problems /*host*/, int count, int layout, int cfg, void* stream);
/* Block tile (BM x BN) the launcher uses for a group with these maximum extents: one EPI_MSE partial is
 * written per tile, tile id = m_tile + tiles_m * n_tile. */
int jamie_gemm_tile(int layout, int max_m, int max_n, int max_k, int cfg, int* bm /*host*/, int* bn /*host*/);

/* ---------------------------------------------------------------------------------------------
 * bf16 compute mode (BASELINE config 2: bf16 compute / fp32 master weights).  Same products as jamie_gemm_f32 as
 * C[M,N] (fp32, or bf16 with c_bf16) = A[M,K] * B[N,K]^T on bf16 operands (A, B of the problem struct point to bf16;
 * lda/ldb in elements; K, lda, ldb multiples of 8; epilogues STORE and MSE), K-contiguous unless a_tr / b_tr say the operand is
 * stored k-row-major (large-tile configurations: the operands are read as their producers stored them, no transposed copies):
 *   forward A = a [B,in], B = W [out,in];  dX: A = dy [B,out], B = W [out,in] with b_tr;  dW: A = dy [B,out] with a_tr,
 *   B = a [B,in] with b_tr.  Small-tile configurations need K-contiguous (transposed) copies: jamie_cast_transpose.
 * ------------------------------------------------------------------------------------------- */
int jamie_gemm_bf16(const jamie_gemm_problem* problems /*host*/, int count, int cfg, void* stream);
int jamie_gemm_bf16_tile(int max_m, int max_n, int cfg, int* bm /*host*/, int* bn /*host*/);
typedef struct {
    const float* src;           /* [R, C] fp32, leading dimension ld, nslab slabs slab_stride apart (summed)   */
    void* dst;                  /* bf16 [R, C] (ldd) or NULL                                                    */
    void* dstT;                 /* bf16 [C, R] (ldt) or NULL                                                    */
    int R, C, ld, ldd, ldt, nslab;
    long long slab_stride;
    const void* src_bf16;       /* alternative source: bf16 [R, C] (ld), with src = NULL and nslab = 1 (a transposed  */
                                /* copy of an existing bf16 matrix, e.g. the weights the Adam kernel wrote)            */
    const int32_t* rows;        /* optional row gather: output row r reads source row rows[r] (x = data[idx],          */
                                /* jamie.py:583: the batch is gathered, cast and transposed in ONE launch)            */
    float* dst32; int ld32;     /* optional fp32 copy [R, C] of the gathered / slab-summed rows                        */
} jamie_cast_problem;
int jamie_cast_transpose(const jamie_cast_problem* problems /*host*/, int count /* <= 16 */, void* stream);

/* Reconstruction loss (jamie.py:637-641) behind a split-K x_hat GEMM: y = sum of `nslab` slabs [R, C] (contiguous,
 * bias already added by the GEMM), d = (y - x) * scale -> fp32 [R, C] and optional bf16 [R, C] / bf16 [C, R] copies;
 * partial[t] = pscale * sum (y - x)^2 over 64x64 tile t (tile index = m_tile + tiles_m * n_tile, the order of the
 * 64x64 GEMM's fused MSE epilogue), ceil(R/64) * ceil(C/64) partials per problem. */
typedef struct {
    const float* y; const float* x; float* d;   /* d: optional (NULL: only the bf16 copies / column sums leave the launch) */
    void* d_bf16; void* dT_bf16;        /* optional */
    float* partial;                     /* optional */
    int R, C, nslab; long long slab_stride;
    float scale, pscale;
    float* colpart;                     /* optional [ceil(R / 64), C]: column sums of d over each 64-row tile (rows added in order): the
                                         * decoder's output-bias gradient = column sums of d x_hat (jamie.py:734) is then a sum of
                                         * ceil(R / 64) rows instead of a second pass over the [R, C] matrix */
} jamie_mse_problem;
int jamie_mse_cast(const jamie_mse_problem* problems /*host*/, int count /* <= JAMIE_MAX_GROUP */, void* stream);

/* one column-sum problem: out[n] (+)= sum_m sum_slabs X[m, n] (jamie_colsum_group; extra workgroups of jamie_bn_act_bwd_cs and
 * jamie_grad_sqnorm_ranges_fin) */
typedef struct { const float* X; float* out; int M, N, ld, nslab; long long slab_stride; int accumulate; } jamie_colsum_problem;
/* ---------------------------------------------------------------------------------------------
 * BatchNorm1d(train) + LeakyReLU + Dropout, forward and backward, one column strip per workgroup.
 * Replaces native_batch_norm / leaky_relu / bernoulli_ + mul (model.py:152-154,162-164,193-195,198-200)
 * and their backward.  h may arrive as `nslab` split-K slabs (summed here; slab 0 receives the sum).
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    float* h; int nslab; long long slab_stride;      /* pre-BN activations [B,N] (in/out: summed)   */
    const float* gamma; const float* beta;
    float* running_mean; float* running_var;         /* updated in place (momentum, unbiased var)   */
    float* save_mean; float* save_invstd;            /* [N] each, for the backward pass             */
    float* out;                                      /* [B,N] activation after dropout              */
    const uint8_t* mask;                             /* explicit 0/1 keep mask [B,N] or NULL (RNG)  */
    int B, N;
    int rng_stream;                                  /* dropout without `mask`: element (row, col) is kept iff a 16-bit half of
                                                      * one Philox4x32-10 word is >= thr = trunc(p * 65536) (fp32 product,
                                                      * clamped to [0, 65535]):
                                                      *   counter = (rk, col >> 2, rng_stream, low 32 bits of rng[1] = step),
                                                      *             rk = (row & 127) | ((row >> 8) << 7)
                                                      *   key     = (low 32 bits of rng[0] = seed, high 32 bits of seed XOR high
                                                      *             32 bits of step)
                                                      *   word col & 3 of the output, its half (row >> 7) & 1 (0: bits 0..15)
                                                      * -- one call serves a quad of columns in rows r and r + 128.  Every kernel
                                                      * (dword / float4, forward / backward) draws the same bit for the same
                                                      * element (tests/bn_util.py keep_mask, tests/test_hip_bn.py).  The keep
                                                      * probability is 1 - trunc(p * 65536) / 65536 (0.4000092 at p = 0.6) while
                                                      * the survivors are scaled by 1 / (1 - p) */
    void* out_bf16;                                  /* optional bf16 [B,N] copy of `out` (out may be NULL) */
    void* outT_bf16;                                 /* optional bf16 transposed [N,B] copy.  Either bf16 copy: B % 8 == 0, and
                                                      * B <= 1024 on the float4 path (N % 4 == 0, slab_stride % 4 == 0, aligned
                                                      * pointers; the transposed tile is 16 x (128 R + 2) shorts of LDS, R = 4 or
                                                      * 8), B <= 512 on the dword path; anything else is an argument error */
    int panel;                                       /* 1: `h` (every slab, and the sum written back to slab 0) is in panels of
                                                      * JAMIE_PANEL columns (jamie_gemm_problem.c_panel); float4 kernels only
                                                      * (B <= 1024, N % 4 == 0); `out` / the bf16 copies / `mask` stay row-major */
} jamie_bnact_fwd_problem;

int jamie_bn_act_fwd(const jamie_bnact_fwd_problem* problems /*host*/, int count, float p_drop,
                     float momentum, float eps, float slope, const uint64_t* rng, void* stream);

/* jamie_bn_act_fwd / jamie_bn_act_bwd_cs with a PREFETCH RIDER: 64 extra workgroups (float4 kernels only; ignored otherwise) read
 * up to 8 device ranges (prefetch[i], prefetch_bytes[i]; 16-byte aligned; host arrays) with the default cache policy and discard
 * them -- what the NEXT launches stream (the weights of the next product, model.py:151 etc.; saved activations of the backward
 * pass) is then in the Infinity Cache instead of HBM-cold.  n_colsums may be 0. */
int jamie_bn_act_fwd_pf(const jamie_bnact_fwd_problem* problems /*host*/, int count, float p_drop, float momentum, float eps,
                        float slope, const uint64_t* rng, const void* const* prefetch /*host*/, const long long* prefetch_bytes /*host*/,
                        int n_prefetch, void* stream);

typedef struct {
    float* da; int nslab; long long slab_stride;     /* grad wrt activation out; dh is written to slab 0 */
    const float* h; const float* gamma; const float* beta;
    const float* save_mean; const float* save_invstd;
    float* dgamma; float* dbeta; float* dbias_lin;   /* [N] each; dbias_lin = colsum(dh) or NULL    */
    const uint8_t* mask;
    int B, N; int rng_stream; int accumulate;        /* accumulate: d{gamma,beta,bias} += */
    void* dh_bf16; void* dhT_bf16;                   /* optional bf16 [B,N] / transposed [N,B] copies of dh */
    int skip_f32;                                    /* 1: do not write the fp32 dh (bf16 copies only)     */
    int panel;                                       /* 1: `da` (every slab) and `h` are in panels of JAMIE_PANEL columns; needs
                                                      * skip_f32 (dh leaves as bf16 row-major only); float4 kernels only */
} jamie_bnact_bwd_problem;

int jamie_bn_act_bwd(const jamie_bnact_bwd_problem* problems /*host*/, int count, float p_drop,
                     float slope, const uint64_t* rng, void* stream);
/* The same launch with EXTRA workgroups that compute column sums (`colsums`: out[n] = sum_m X[m, n]; e.g. the decoder's
 * output-bias gradient, the column sums of d x_hat, jamie.py:734): a job of 47 short workgroups that would otherwise be a launch
 * of its own at the head of the backward pass runs beside this launch's long ones. */
int jamie_bn_act_bwd_cs(const jamie_bnact_bwd_problem* problems /*host*/, int count, float p_drop, float slope,
                        const uint64_t* rng, const jamie_colsum_problem* colsums /*host*/, int n_colsums, void* stream);
/* ... and with the prefetch rider of jamie_bn_act_fwd_pf (n_colsums may be 0) */
int jamie_bn_act_bwd_pf(const jamie_bnact_bwd_problem* problems /*host*/, int count, float p_drop, float slope, const uint64_t* rng,
                        const jamie_colsum_problem* colsums /*host*/, int n_colsums, const void* const* prefetch /*host*/,
                        const long long* prefetch_bytes /*host*/, int n_prefetch, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Latent block: reparameterisation (model.py:225-243), sigma-weighted combine (model.py:245-259),
 * KL / alignment ("CosSim") / F losses and their gradients (jamie.py:618-668), two modalities.
 * All [B,L] matrices are dense row-major with ld = L except `ml` / `dml` ([B,2L]: mu | logvar).
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    int B, L;
    /* inputs */
    const float* ml[2]; int ml_nslab; long long ml_slab_stride;  /* heads GEMM output slabs [B,2L]   */
    const float* head_bias[2];                                   /* [2L]: b_mu | b_var                */
    const float* eps_in[2];          /* explicit N(0,1) noise [B,L] or NULL -> drawn from `rng`       */
    const float* sigma;              /* [2] */
    const float* corr;               /* [B,B] or NULL (= identity)                                    */
    const float* Fblk;               /* [B,B] row-normalised F block or NULL (= 0)                     */
    const float* hyper;              /* device float[16]: [0] kl_scale (= w_kl*32e-3*anneal), [1] w_rec, [2] w_align
                                        (= w_cos*32), [3] w_f; [8..13] = Adam block (see jamie_clip_adam)           */
    /* saved forward state (device, caller-owned) */
    float* mu[2]; float* lv[2]; float* z[2]; float* eps[2]; float* comb[2];
    float* cz[2];                    /* cz[0] = C z1, cz[1] = C^T z0                                   */
    float* rsum; float* qsum;        /* rowsum(C), colsum(C) [B]                                       */
    float* fc1;                      /* F comb1 [B,L]                                                  */
    float* partials;                 /* fp32 scratch, >= jamie_max_partials() * 16                     */
    /* backward */
    const float* dcomb[2]; int dcomb_nslab; long long dcomb_slab_stride; /* from decoder dX GEMM     */
    float* H[2]; float* ch[2];       /* scratch [B,L]: H_i = G_i / den_i;  ch[0] = C H1, ch[1] = C^T H0 */
    float* fte;                      /* scratch [B,L]: F^T E                                          */
    float* dml[2];                   /* out: d(mu|logvar) [B,2L]                                      */
    float* dsigma;                   /* out: [2]                                                       */
    const float* rec_partials; int n_rec_partials;  /* MSE partials from the decoder GEMM epilogue   */
    float* losses;                   /* out: device float[8]: KL, Rec, CosSim, F (weighted), total, running min(total) */
    int cosine;                      /* dist_method == 'cosine' (jamie.py:484-494)                    */
    int rng_stream;
    /* optional external upstream gradients [B,L] (autograd seam: the caller computes its own losses on the
       forward outputs, reference jamie.py:611-734); added to the internally derived ones; NULL = none.
       An external d(combined) is passed as one more `dcomb` slab.                                     */
    const float* dz_ext[2]; const float* dmu_ext[2]; const float* dlv_ext /* last modality's logvar */;
    /* optional bf16 copies for the bf16 compute mode (NULL = none): comb [B,L] / [L,B], d(mu|logvar) [B,2L] / [2L,B] */
    void* comb_bf16[2]; void* combT_bf16[2]; void* dml_bf16[2]; void* dmlT_bf16[2];
} jamie_latent;

int jamie_latent_fwd(const jamie_latent* a /*host*/, const uint64_t* rng, void* stream);
int jamie_latent_bwd(const jamie_latent* a /*host*/, void* stream);

/* M-modality latent block (2 <= M <= 4) for fully paired cells: identity correspondence, F = 0, euclidean alignment.
 * The reference supports two modalities only (jamie.py:420, model.py:251-256); this is the build-defined
 * generalisation of SURVEY.md §8 row A14 (comb = sum_j sigma_j z_j / sum_j sigma_j; KL rows 0..M-1 of the last
 * modality's logvar).  For M = 2 it equals jamie_latent_* at corr = NULL and is the path the training step takes for
 * identity correspondence.  L: a multiple of 4, <= 128.  Pointer arrays are indexed by modality. */
typedef struct {
    int B, L, M;
    const float* ml[4]; int ml_nslab; long long ml_slab_stride;
    const float* head_bias[4]; const float* eps_in[4];
    const float* sigma; const float* hyper;
    float* mu[4]; float* lv[4]; float* z[4]; float* eps[4];
    float* comb;                     /* [B,L]: identical for every modality                              */
    float* partials;                 /* fp32 scratch, >= jamie_max_partials() * 17                       */
    const float* dcomb[4]; int dcomb_nslab; long long dcomb_slab_stride;
    float* dml[4]; float* dsigma;    /* dsigma [M]                                                        */
    const float* rec_partials; int n_rec_partials; float* losses;
    int rng_stream;
    /* fused tail (all optional, NULL = off).  Forward: the SAME launch computes decoder layer 0 of every modality,
     * g1_i [B, d_i] = comb dec0_W_i^T + dec0_b_i (reference model.py:190; exact fp32 on the vector ALU: K = L), stores comb
     * into every `comb_alias[i]` and the bf16 copies the bf16 GEMMs of the backward pass read.  Backward: bf16 copies of
     * d(mu | logvar) and the head-bias gradients dbias_head[i] [2L] = column sums of dml_i ((+)= when `accumulate`),
     * which need `colpart` (jamie_latent_m_colpart_size() floats). */
    float* g1[4]; const float* dec0_W[4] /* [d_i, L] */; const float* dec0_b[4]; int d[4];
    float* comb_alias[4];
    void* comb_bf16[4] /* [B, L] */; void* combT_bf16[4] /* [L, B] */;
    void* dml_bf16[4] /* [B, 2L] */; void* dmlT_bf16[4] /* [2L, B] */;
    float* dbias_head[4]; float* colpart; int accumulate;
    unsigned* ticket;   /* REQUIRED for the backward launch unless defer_final: one zero-initialised device uint32 (count of
                         * finished workgroups; the last one finalises the losses, d sigma and the head-bias gradients and
                         * resets it) */
    int defer_final;    /* 1: jamie_latent_m_bwd leaves the partial sums as they are; the step's range-norm launch finalises
                         * them in an extra workgroup (jamie_grad_sqnorm_ranges_fin), off the backward pass's critical path */
    /* optional fused tail of jamie_latent_m_bwd: da2[i] [B, d[i]] (fp32, ld = d[i]) = d(mu | logvar)_i [B, 2L] head_W[i] [2L, d[i]]
     * -- the heads' input gradient (dx of nn.Linear(d, 2L), model.py:141-143) computed by extra workgroups of the same launch
     * in exact fp32; d[i] a multiple of 4.  NULL: the caller runs that product as a GEMM. */
    const float* head_W[4]; float* da2[4];
    /* optional by-product of jamie_latent_m_fwd's fused tail (g1 given): the K-contiguous bf16 copy dec0_WT_bf16[i] [L, d[i]] of
     * W_dec0 [d[i], L], written by the workgroups that stage the weight chunks anyway; what jamie_gemm_bf16_skinny multiplies
     * d g1 by for the decoder-layer-0 input gradient (d[i] a multiple of 8).  NULL: not written. */
    void* dec0_WT_bf16[4];
    int g1_panel, da2_panel;    /* 1: g1[i] / da2[i] are written in panels of JAMIE_PANEL columns (see jamie_gemm_problem.c_panel):
                                 * what the BatchNorm launches that consume them read when their `panel` is set */
} jamie_latent_m;
/* What a riding sampler draws: idx[B] = jamie_sample_indices(B, N, offset, replace, {seed, step + step_add}, rng_stream)
 * (np.random.choice of jamie/jamie.py:556).  step_add = 1 in a launch that runs before the norm kernel has advanced the step. */
typedef struct { int32_t* idx; int B; long long N; long long offset; int replace; int rng_stream; int step_add; } jamie_sample_args;
/* forward: ONE launch from the heads' split-K slabs to mu / logvar / z / comb, the loss partial sums and (fused tail) the
 * decoder's first pre-activation; backward: ONE launch (gradients + partial sums; its last workgroup finalises the losses, d sigma
 * and the head-bias gradients) */
int jamie_latent_m_fwd(const jamie_latent_m* a /*host*/, const uint64_t* rng, void* stream);
int jamie_latent_m_bwd(const jamie_latent_m* a /*host*/, void* stream);
/* jamie_latent_m_bwd with ONE extra workgroup that draws the NEXT step's batch indices (sample->step_add = 1: the norm kernel
 * has not advanced the step yet): early enough for the batch gather to ride in the optimiser launch (jamie_clip_adam_ride) */
int jamie_latent_m_bwd_ex(const jamie_latent_m* a /*host*/, const jamie_sample_args* sample /*host*/, const uint64_t* state, void* stream);
long long jamie_latent_m_colpart_size(int B, int L);

/* ---------------------------------------------------------------------------------------------
 * Optimiser: global-norm clip + Adam on one flat fp32 buffer
 * (clip_grad_norm_(params, 1) + optim.Adam.step + zero_grad, jamie.py:739-741).
 * `state` = device uint64[4] shared with `rng`: state[1] (step) is incremented by jamie_grad_sqnorm.
 * hyper (device float[16], shared with jamie_latent): [8] lr, [9] beta1, [10] beta2, [11] eps, [12] max_norm,
 * [13] grad_scale (1/world_size: the all-reduced SUM is averaged inside the update),
 * [14] 1 - beta1, [15] 1 - beta2: formed in double by the host and rounded once, as torch.optim.Adam forms them (1 - 0.999 rounds
 * to 0.001f; 1.f - fl32(0.999) is 1.29e-5 smaller).  Used for the moment updates and, as 1 - (double)hyper[14|15], for the bias
 * corrections.  A slot that is 0 means "not given": the kernel then forms 1.f - beta itself.
 * A NaN gradient norm gives a NaN clip coefficient (every p, m, v becomes NaN), as clip_grad_norm_ does.
 * ------------------------------------------------------------------------------------------- */
int jamie_optim_blocks(long long n);   /* number of partials jamie_grad_sqnorm writes for n elements */
int jamie_grad_sqnorm(const float* g, long long n, float* partials, int n_partials, uint64_t* state,
                      void* stream);
/* The same over `count` ranges [offsets[i], offsets[i] + lengths[i]) of g only: one partial per chunk of 4096
 * elements, or of the smallest multiple of 4096 that keeps the chunk count at <= 128 (jamie_sqnorm_range_blocks() of them).  Used with the dW launches of jamie_gemm_bf16 that write
 * the sum of squares of every stored tile into `partial` (EPI_STORE + partial): together they cover the gradient, and
 * jamie_clip_adam sums all of them -- clip_grad_norm_ (jamie.py:739) without a second pass over the weight gradients. */
int jamie_grad_sqnorm_ranges(const float* g, const long long* offsets /*host*/, const long long* lengths /*host*/, int count,
                             float* partials, int n_partials, uint64_t* state, void* stream);
/* The same, and additionally g_bf16[i] = bf16(g[i]) over those ranges (same offsets): with the dW launches writing bf16
 * (jamie_gemm_problem.c_bf16) the whole gradient then exists in ONE bf16 buffer for jamie_clip_adam_g16. */
int jamie_grad_sqnorm_ranges_g16(const float* g, void* g_bf16, const long long* offsets /*host*/, const long long* lengths /*host*/,
                                 int count, float* partials, int n_partials, uint64_t* state, void* stream);
/* jamie_grad_sqnorm_ranges (g_bf16 NULL) / _g16 plus extra workgroups for work that would otherwise be launches of its own on
 * the step's critical path: ONE that finalises a deferred latent backward pass (`fin->defer_final`): losses, d sigma, head-bias
 * gradients (written into g, and g_bf16) and their sum of squares into partials[range blocks]; and, optionally, column sums
 * (`colsums`, e.g. the decoder's output-bias gradient = column sums of d x_hat, jamie.py:734), each workgroup of 64 columns
 * writing its sums into g (and g_bf16) and their squares into the next partial.  The ranges must NOT cover what the extra
 * workgroups write; n_partials = range blocks + 1 + sum(ceil(N_i / 64)). */
int jamie_grad_sqnorm_ranges_fin(const float* g, void* g_bf16, const long long* offsets /*host*/, const long long* lengths /*host*/,
                                 int count, float* partials, int n_partials, uint64_t* state,
                                 const jamie_latent_m* fin /*host*/, const jamie_colsum_problem* colsums /*host or NULL*/,
                                 int n_colsums, void* stream);
/* jamie_gemm_bf16 (tile configuration 29: the dW launches) + jamie_grad_sqnorm_ranges_fin (without column sums) in ONE launch:
 * the range chunks and the finaliser run as extra workgroups behind the GEMM tiles.  For the LAST dW launch of a backward pass:
 * every gradient the ranges cover must be complete before the launch.  `fin` may be NULL (n_partials = range blocks). */
int jamie_gemm_bf16_ranges(const jamie_gemm_problem* problems /*host*/, int count, int cfg, const float* g, void* g_bf16,
                           const long long* offsets /*host*/, const long long* lengths /*host*/, int n_ranges, float* partials,
                           int n_partials, uint64_t* state, const jamie_latent_m* fin /*host or NULL*/, void* stream);
int jamie_sqnorm_range_blocks(const long long* lengths /*host*/, int count);
int jamie_clip_adam(float* p, const float* g, float* m, float* v, long long n, const float* partials,
                    int n_partials, const float* hyper, const uint64_t* state,
                    void* p_bf16 /* optional bf16 copy of the updated parameters (same layout) or NULL */, void* stream);
/* The same two steps on a bf16 gradient: the reduced gradient of the data-parallel exchange is left in its bf16 message
 * buffer (same offsets as the flat fp32 gradient) and read from there -- no fp32 copy-back pass, 2 instead of 4 bytes of
 * gradient per parameter in both kernels. */
int jamie_grad_sqnorm_bf16(const void* g_bf16, long long n, float* partials, int n_partials, uint64_t* state, void* stream);
/* jamie_clip_adam (g fp32) / jamie_clip_adam_g16 (g_is_bf16) with EXTRA workgroups that do work of the NEXT step, which would
 * otherwise be launches of its own on the critical path, beside the 256 streaming workgroups of this ~190 us launch: either the
 * next batch's sampler (`sample`; state[1] already holds the next step's number: step_add = 0) or the next batch's row gather +
 * bf16 cast (`casts`: jamie_cast_transpose problems; the batch buffers are free once the step's last dW product has run) --
 * not both: the gather reads the sampler's output. */
int jamie_clip_adam_ride(float* p, const void* g, int g_is_bf16, float* m, float* v, long long n, const float* partials,
                         int n_partials, const float* hyper, const uint64_t* state, void* p_bf16,
                         const jamie_sample_args* sample /*host or NULL*/, const jamie_cast_problem* casts /*host or NULL*/,
                         int n_casts, void* stream);
int jamie_clip_adam_g16(float* p, const void* g_bf16, float* m, float* v, long long n, const float* partials,
                        int n_partials, const float* hyper, const uint64_t* state, void* p_bf16, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Batch assembly (jamie.py:552-604).
 * ------------------------------------------------------------------------------------------- */
/* dst[b,:] = src[idx[b],:]   (`dataset[i][random_batch[i]]`, jamie.py:583) */
int jamie_gather_rows(const float* src, long long n_rows, int d, const int32_t* idx, int B, float* dst,
                      void* stream);
/* Uniform B-subset of [0,N) without replacement (replace=0) or B draws with replacement, from `rng`
 * (device-side counterpart of np.random.choice, jamie.py:556); one workgroup, deterministic. */
int jamie_sample_indices(int32_t* idx, int B, long long N, long long offset, int replace,
                         const uint64_t* rng, int rng_stream, void* stream);
/* up to 4 independent draws in one launch (one workgroup each): the hybrid sampler's pair numbers and rows of both modalities */
int jamie_sample_indices_group(const jamie_sample_args* list /*host*/, int count, const uint64_t* rng, void* stream);
/* 'hybrid' sampler of partial-correspondence training on the device (jamie.py:559-573, corrected): slot b is, with
 * probability true_ratio, known pair pairs[pidx[b] % num_corr] = (row of modality 0, row of modality 1), else (r0[b], r1[b]);
 * true_ratio = 1 pairs every slot; pidx / r0 / r1: candidate draws from jamie_sample_indices */
int jamie_hybrid_assemble(const int32_t* pairs /*[num_corr,2]*/, const int32_t* pidx, const int32_t* r0, const int32_t* r1,
                          int B, int num_corr, float true_ratio, const uint64_t* rng, int rng_stream, int32_t* idx0,
                          int32_t* idx1, void* stream);
/* corr[a,b] = (idx0[a] == idx1[b]) row-normalised (P = I_N block, jamie.py:586-589) */
int jamie_corr_from_indices(const int32_t* idx0, const int32_t* idx1, int B, float* corr, void* stream);
/* blk[a,b] = P[idx0[a] + row_off, idx1[b] + col_off] for P in CSR form (int32 indptr / indices sorted within each
 * row, fp32 values; `indices` / `vals` may be NULL when the matrix has no entries), row-normalised when `normalise`
 * (zero rows keep divisor 1): P[idx0][:, idx1] of jamie.py:586-589 for sparse partial correspondence, no N x N array. */
int jamie_csr_block(const int32_t* indptr, const int32_t* indices, const float* vals, const int32_t* idx0,
                    const int32_t* idx1, int B0, int B1, int row_off, int col_off, int normalise, float* out /*[B0,B1]*/,
                    void* stream);
/* out[a,b] = w_blk * blk[a,b] + w_add * add[a,b] with blk = M[idx0[a] + row_off, idx1[b] + col_off] of a DENSE row-major
 * matrix (leading dimension ld), row-normalised when `normalise` (zero rows keep divisor 1); `add` may be NULL.
 * Replaces P[idx0][:, idx1] / F[idx0][:, idx1], their row normalisation and the mix corr = PF_Ratio * P + (1 - PF_Ratio) * F
 * of jamie/jamie.py:586-604 (the reference first gathers a [B, N] slab). */
int jamie_dense_block(const float* M, long long ld, const int32_t* idx0, const int32_t* idx1, int B0, int B1,
                      long long row_off, long long col_off, int normalise, float w_blk, const float* add /*[B0,B1] or NULL*/,
                      float w_add, float* out /*[B0,B1]*/, void* stream);
/* out[i] = a * x[i] + b * y[i] (y may be NULL): PF_Ratio * P + (1 - PF_Ratio) * F on [B,B] blocks (jamie/jamie.py:604) */
int jamie_axpby(float* out, float a, const float* x, float b, const float* y, long long n, void* stream);
/* out[n] (+)= sum_m X[m,n]  (bias gradients of the non-BN Linear layers) */
int jamie_colsum(const float* X, int M, int N, int ld, int nslab, long long slab_stride, float* out,
                 int accumulate, void* stream);
/* the same for up to JAMIE_MAX_GROUP matrices in one launch (the modalities) */
int jamie_colsum_group(const jamie_colsum_problem* problems /*host*/, int count, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Correspondence stage: JAMIE.Prime_Dual (jamie/jamie.py:314-414, MultiOmics branch), SURVEY.md §8(f) rank 3.
 * The seven dense products per iteration of the reference become four jamie_gemm_f32 launches issued by the
 * host (T1 = F^T (F Ky), G1 = (F Ky) T1, F Ky and G2 = Kx (F Ky) for the new F); the element-wise rest of one
 * iteration is the two entry points below.  All matrices are contiguous row-major fp32 on the device.
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    float* F;            /* [m,n] correspondence matrix, updated in place (jamie.py:339, 384) */
    const float* G1;     /* [m,n] (F Ky)(F^T F Ky) for the current F (jamie.py:358-359) */
    const float* G2;     /* [m,n] Kx F Ky for the current F (jamie.py:360) */
    float* m1;           /* [m,n] first / second moment (jamie.py:350-351, 376-377) */
    float* m2;
    float* Mu;           /* [m]  dual variable (jamie.py:343, 393) */
    float* Lambda;       /* [n]  dual variable (jamie.py:342, 394) */
    float* S;            /* [n]  slack (jamie.py:344, 386-390) */
    float* rowsum;       /* [m]  F 1   of the current F, replaced by that of the new F */
    float* colsum;       /* [n]  F^T 1 of the current F, replaced by that of the new F */
    const float* alpha;  /* [1]  scaling factor a (jamie.py:335, 397-402) */
    float* rowpart;      /* workspace, jamie_pd_workspace() elements */
    float* colpart;
    int m, n;
    float rho, epsilon;  /* UnionCom attributes (jamie.py:365, 384) */
} jamie_pd_state;
/* sizes (in floats) of the two partial-sum workspaces for an [m,n] problem */
int jamie_pd_workspace(int m, int n, long long* rowpart_elems, long long* colpart_elems);
/* One iteration's element-wise work (jamie.py:357-394 minus the products): gradient from G1, G2 and the rank-one
 * terms, moments with bias correction for `iteration` (1-based), projected step, F <- (1-eps) F + eps relu(F - step),
 * then row / column sums of the new F and the S, Mu, Lambda updates.  Deterministic (no atomics). */
int jamie_pd_step(const jamie_pd_state* state /*host*/, int iteration, void* stream);
/* alpha[0] = sum(G2 o F) * inv_trkk = tr(Kx (F Ky) F^T) / tr(Kx Kx) for G2 = Kx F Ky (jamie.py:397-402);
 * `partials`: n_partials <= 4096 floats of workspace */
int jamie_pd_alpha(const float* G2, const float* F, long long count, float* partials, int n_partials, float inv_trkk,
                   float* alpha, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Device-side preprocessing: `preclass(sample, axis=0)` of the reference (utilities.py:654-678; built at
 * jamie.py:462-465, applied at jamie.py:508), SURVEY.md §8(f) rank 4.  X is [N, d] row-major fp32 (is_f64 = 0) or
 * fp64 (is_f64 = 1) on the device.
 * ------------------------------------------------------------------------------------------------ */
/* mean[d], sd[d] (fp64; population standard deviation, numpy's two-pass order); `partials`: n_row_blocks * d doubles */
int jamie_col_stats(const void* X, int is_f64, long long N, int d, long long ld, double* partials, int n_row_blocks,
                    double* mean, double* sd, void* stream);
/* out[N,d] fp32 = (X - mean) / sd computed in fp64, NaN -> 0 (utilities.py:663-669) */
int jamie_standardise(const void* X, int is_f64, long long N, int d, long long ld, const double* mean, const double* sd,
                      float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Stage A distances on the device (jamie_amd/distances.py; reference `compute_distances`, jamie.py:839-890, and unioncom's
 * geodesic_distances, jamie_amd/utilities.py).  D is one N x N fp32 buffer, row-major with ld = N, used in place by every call
 * below; X is the column-centred data [N, d] fp32 (jamie_col_stats + jamie_standardise with sd = 1) and G = X X^T comes from
 * jamie_gemm_f32_cfg (JAMIE_NT, configuration 17) written into D.  Deterministic: no floating-point atomics.
 * ------------------------------------------------------------------------------------------------ */
/* floats of `partials` jamie_apsp_finalise needs for N cells */
long long jamie_dist_workspace(long long N);
/* out[i] = sum_c X[i, c]^2 (fp32) */
int jamie_row_sqnorm(const float* X, long long N, int d, float* out, void* stream);
/* D = G -> sqrt(q) (squared = 0) or q (squared = 1), q = max(n_i + n_j - 2 G_ij, 0), diagonal exactly 0, exactly symmetric (both
 * halves from the upper triangle of G): sklearn `pairwise_distances(metric='euclidean' | 'sqeuclidean')`.  Where cancellation
 * dominates, q < 2^-10 (n_i + n_j) (near-duplicate cells), q is recomputed as sum_c (X[i, c] - X[j, c])^2 in fp32 from X [N, d],
 * the rows sqnorm was taken of: |dD| <= 1.35e-6 c max D for a summation-noise factor c ~ 1, exact duplicates exactly 0 */
int jamie_gram_to_distances(float* D, const float* sqnorm, const float* X, long long N, int d, int squared, void* stream);
/* out[i, :] = (X[i, :] - m_i) / |X[i, :] - m_i| as fp32 [N, d], m_i = the mean of row i (centre = 1) or 0 (centre = 0); mean, norm and
 * quotient in fp64, one rounding at the store.  X is fp32 (is_f64 = 0) or fp64 (1), NOT column-centred.  norm[i] = the norm as fp32,
 * exactly 0 for a zero row and, with centre = 1, for a constant row (every entry equal); such a row is written as zeros: the rows
 * sklearn `normalize` leaves alone and scipy's `correlation` / `np.corrcoef` turn into NaN */
int jamie_row_normalise(const void* X, int is_f64, long long N, int d, int centre, float* out, float* norm, void* stream);
/* D = G -> scale * q for unit rows: X = the rows U of jamie_row_normalise, column-centred like the euclidean input (|u - v|^2 does
 * not change under a shift), G = X X^T, sqnorm = jamie_row_sqnorm(X), rownorm = jamie_row_normalise's norm.  q and its recompute as
 * in jamie_gram_to_distances (1 - u.v = |u - v|^2 / 2), diagonal exactly 0, exactly symmetric; where either row is a zero row
 * (rownorm == 0) D = 1 off the diagonal.  scale = 1/2 with centre = 0: sklearn `pairwise_distances(metric='cosine')`; 1/2 with
 * centre = 1: `pairwise_distances(metric='correlation')`; 1/4 with centre = 1: `(1 - np.corrcoef(X)) / 2` (utilities.distance_matrix
 * 'pearson').  scale must be positive and finite */
int jamie_gram_to_scaled_sqdist(float* D, const float* sqnorm, const float* X, long long N, int d, float scale, const float* rownorm,
                                void* stream);
/* D[i, j] = sum_c |X[i, c] - X[j, c]| (op = 0) or max_c |X[i, c] - X[j, c]| (op = 1) in fp32 by direct difference over all pairs of
 * X [N, d], every entry of the N x N buffer written (no Gram matrix): sklearn `pairwise_distances(metric='manhattan' | 'l1' |
 * 'cityblock')` and `(metric='chebyshev')`.  One chain per pair in ascending c, sums in chunks of 32 features; diagonal exactly 0,
 * exactly symmetric, exact where the differences and their sums are fp32 numbers.  Any other op returns an error before a launch.
 * Long pair spaces are split over several launches inside the call */
int jamie_pairwise_absdiff(const float* X, long long N, int d, int op, float* D, void* stream);
/* idx[i, 0] = i, idx[i, 1 .. K) = the K - 1 smallest off-diagonal entries of row i of D, ascending (ties: lower column first); radix
 * select on the fp32 bits (D >= 0), survivors sorted.  1 <= K <= min(N, 1024): sklearn
 * `NearestNeighbors(n_neighbors=K).fit(X).kneighbors_graph(X)` (X given explicitly, so the cell is its own first neighbour) */
int jamie_knn_topk(const float* D, long long N, int K, int32_t* idx, void* stream);
/* w[i, s] = sqrt(sum_c (X[i, c] - X[idx[i, s], c])^2) in fp32: the kNN graph's edge weights by direct difference */
int jamie_knn_weights(const float* X, long long N, int d, const int32_t* idx, int K, float* w, void* stream);
/* D = +inf, diagonal 0, then every edge (i, idx[i, s]) with s < k (of the K columns of idx / w) to D_ij and D_ji, the smaller weight
 * kept: the graph csgraph `shortest_path(kneighbors_graph, directed=False)` walks */
int jamie_knn_graph_init(float* D, long long N, const int32_t* idx, const float* w, int K, int k, void* stream);
/* all-pairs shortest paths in place, blocked Floyd-Warshall on 128 x 128 blocks (rows / columns past N act as +inf padding):
 * csgraph `shortest_path(method='D', directed=False)` */
int jamie_apsp_fw(float* D, long long N, void* stream);
/* D = min(D, D^T); maxv[0] = the largest finite entry (0 if none); every +inf -> 2 maxv[0] (utilities.geodesic_distances' last
 * step).  `partials`: n_partials >= jamie_dist_workspace(N) floats */
int jamie_apsp_finalise(float* D, long long N, float* partials, long long n_partials, float* maxv, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Alignment metrics on the device (jamie_amd/metrics.py; reference `test_closer`, jamie.py:892-915, and `test_LabelTA`,
 * jamie.py:943-961).  All pairs between two fp32 [N, L] row-major embeddings, reduced on the fly to O(N) numbers: nothing of size
 * N x N is stored.  q(i, j) = sum_c (X[i, c] - Y[j, c])^2 by direct difference in fp32, accumulated in ascending c -- one
 * instruction chain for every q, so equal operands give equal bits; exact on integer-valued data.  Deterministic: integer adds
 * only.  Long pair spaces are split over several launches inside one call.
 * ------------------------------------------------------------------------------------------------ */
/* bytes of `ws` for jamie_cross_knn(Nq, Nr, K); for jamie_foscttm_counts on N cells ask with (N, N, 0) */
long long jamie_metrics_workspace(long long Nq, long long Nr, int K);
/* Cell i of A is paired with cell i of B.  row_closer[i] = #{ j != i : q(i, j) < q(i, i) }, col_closer[j] = #{ i != j : q(i, j) <
 * q(j, j) }, int32 [N] each, from one pass over the pair space (strict <; j = i excluded by index): the two sums of the loop of
 * `test_closer` (`ld < ld[i]` over `d[i][size:]` and over `d[size + i][:size]`), FOSCTTM = (sum row_closer + sum col_closer) /
 * (2 N^2).  q(i, i) is taken first, by the chain of the pair tiles, into ws (N floats) */
int jamie_foscttm_counts(const float* A, const float* B, long long N, int L, int32_t* row_closer, int32_t* col_closer, void* ws,
                         long long ws_bytes, void* stream);
/* For every row of Q [Nq, L] the K rows of R [Nr, L] nearest to it, ascending by (distance, then lower index of R): idx int32
 * [Nq, K], dist fp32 [Nq, K] = sqrt(q), 1 <= K <= min(Nr, 64) (anything else returns an error before a launch): sklearn
 * `NearestNeighbors(n_neighbors=K).fit(R).kneighbors(Q)`.  A workgroup keeps the running lists of its 128 (K <= 16) or 64 queries on
 * chip while it walks its share of R through LDS; the shares' lists are merged in share order */
int jamie_cross_knn(const float* Q, long long Nq, const float* R, long long Nr, int L, int K, int32_t* idx, float* dist, void* ws,
                    long long ws_bytes, void* stream);
/* pred[q] = the class code most frequent among ref_codes[idx[q, 0 .. K)] (0 <= code < n_classes), the lowest such code on a tie:
 * sklearn `KNeighborsClassifier(weights='uniform').predict` with the classes in `np.unique` order */
int jamie_knn_vote(const int32_t* idx, long long Nq, int K, const int32_t* ref_codes, int n_classes, int32_t* pred, void* stream);
/* Silhouette widths (jamie_amd/metrics.py `silhouette`; sklearn `silhouette_samples`) from distance sums per (cell, class).
 * bytes of `ws` for jamie_label_distance_sums (host arithmetic only, no device needed): the work list plus the segments' partial
 * sums, for any class sizes that add up to Nr.  seg_tiles = 0: the library's choice, which depends on Nr alone.  0 for Nq, Nr,
 * C < 1 or seg_tiles < 0 */
long long jamie_label_sums_workspace(long long Nq, long long Nr, int C, int seg_tiles);
/* S[i, c] = sum over the rows j of class c of sqrt(q(i, j)), fp64 [Nq, ldS], ldS >= C (columns at or beyond C are not written).
 * R [Nr, L] holds its rows SORTED BY CLASS: class c is rows [class_off[c], class_off[c + 1]), class_off int64 [C + 1] on the device,
 * from 0 to Nr, not decreasing.  An empty class gives exactly 0; q(i, i) of identical rows is exactly 0, so a cell that is also a row
 * of R adds nothing to its own class.  A workgroup walks 128-row tiles of one class (only the last one masked); sqrt(q) is added
 * over a thread's 8 columns in fp32, then in fp64: relative error of S at most (L / 2 + 9) 2^-24.  No floating-point atomics:
 * bit-identical from run to run, and row i's bits do not depend on where it sits in Q or on Nq.  Classes longer than seg_tiles
 * tiles are cut into segments whose partials (in ws) are added in segment order; seg_tiles = 0: chosen by the library.  class_off
 * is copied to the host, checked there and turned into the work list before the first launch: the call waits for `stream`.
 * L < 1, C < 1, ldS < C, seg_tiles < 0, ws_bytes below jamie_label_sums_workspace(Nq, Nr, C, seg_tiles) or a class_off that does
 * not end at Nr return an error before any kernel is launched */
int jamie_label_distance_sums(const float* Q, long long Nq, const float* R, long long Nr, int L, const long long* class_off, int C,
                              double* S, long long ldS, int seg_tiles, void* ws, long long ws_bytes, void* stream);
/* out[i] (fp64 [Nq]) = the silhouette width of cell i among the classes [win0[i], win0[i] + wlen) (win0 int32 [Nq]; NULL: 0 for
 * every cell; the window is clipped to [0, ldS)), own[i] (int32) its class, counts int64 [ldS] the class sizes:
 * a = S[i, own] / (counts[own] - 1), b = min over the other non-empty classes c of the window of S[i, c] / counts[c],
 * s = (b - a) / max(a, b); NaN where the window holds no other non-empty class (or own[i] is outside [0, ldS)), else 0 where
 * counts[own] == 1 (sklearn's rule) or max(a, b) == 0.  One thread per cell, fp64 */
int jamie_silhouette_widths(const double* S, long long ldS, long long Nq, const long long* counts, const int32_t* own,
                            const int32_t* win0, int wlen, double* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Neighbourhoods on the device (jamie_amd/neighbors.py): the K nearest OTHER rows of one fp32 [N, L] row-major matrix, K <= 128,
 * and the local inverse Simpson index (LISI, Korsunsky et al. 2019) on such lists.  q as in "Alignment metrics on the device": the
 * same chain, exact on integer-valued data.  Nothing of size N x N is stored.  Deterministic: no floating-point atomics, every
 * order fixed by position; bit-identical from run to run.
 * ------------------------------------------------------------------------------------------------ */
/* bytes of `ws` for jamie_self_knn(N, K, seg_rows): the segments' lists, S N min(K, 64) (q, index) pairs for S segments, plus one
 * floor key per row for K > 64.  0 for N < 2, K outside 1 .. 128 or a seg_rows that jamie_self_knn refuses */
long long jamie_self_knn_workspace(long long N, int K, long long seg_rows);
/* For every row i of X [N, L] the K rows j != i nearest to it, ascending by (q(i, j), then lower j): idx int32 [N, K], dist fp32
 * [N, K] = sqrtf(q).  Row i is excluded BY INDEX: a row identical to row i is a neighbour at distance 0 like any other.
 * 1 <= K <= min(N - 1, 128), L >= 1.  K <= 64 is one pass of the workgroup of jamie_cross_knn (lists of 16 up to K = 16, of 64
 * beyond); 64 < K is a second pass that admits only what lies above the row's 64th key (q, index) and selects the K - 64 smallest
 * of that: (q, index) is a total order and both passes form q alike, so the two lists together are exactly the K smallest.
 * seg_rows: rows of X per segment of the walked side, 0 (the library's choice) or a positive multiple of 128; the segments' lists
 * are merged in segment order and the result does not depend on seg_rows.  Anything else, more than 65535 segments or a ws below
 * jamie_self_knn_workspace(N, K, seg_rows) returns an error before a launch */
int jamie_self_knn(const float* X, long long N, int L, int K, int32_t* idx, float* dist, long long seg_rows, void* ws,
                   long long ws_bytes, void* stream);
/* LISI of N cells from their neighbour lists idx int32 [N, K], dist fp32 [N, K] (jamie_self_knn; entries of idx in [0, N), one
 * outside is read as category -1) under n_sets sets of category codes, codes int32 [n_sets, N] (any values): lisi fp64 [n_sets, N],
 * tries int32 [N] (may be NULL) the bisection steps taken.  `compute_simpson_index` of the LISI package in fp64: with D the
 * cell's distances as double, from beta = 1: P_j = exp(-D_j beta), s = sum P, H = log(s) + beta sum(D_j P_j) / s and P_j /= s (H = 0,
 * P = 0 where s == 0); while |H - log(perplexity)| > 1e-5 and fewer than 50 tries, beta is doubled / halved until bracketed, then
 * bisected.  LISI = 1 / sum over the categories of (sum of P_j over the neighbours of that category)^2, formed as sum_e P_e (sum
 * over f with code_f == code_e of P_f); NaN in every set where the final H == 0 (every weight underflowed).  One solve per cell
 * feeds all sets.  One wave per cell, lane l holding neighbours l and l + 64, sums by a fixed lane tree.  K < 2, K > 128, n_sets
 * outside 1 .. 4 or a perplexity outside (1, K) return an error before a launch */
int jamie_lisi(const int32_t* idx, const float* dist, long long N, int K, const int32_t* codes, int n_sets, double perplexity,
               double* lisi, int32_t* tries, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Layout quality on the device (jamie_amd/coranking.py): where the entries of a neighbour list -- made in another space of the
 * same cells -- rank in the space X, fp32 [N, L] row-major: what trustworthiness, continuity and the co-ranking curve Q_NX are
 * sums of.  q and the order (q ascending, then the lower index) as in "Neighbourhoods on the device": an entry that
 * jamie_self_knn on X puts at list position p has rank p.  Nothing of size N x N is stored.  Integer counts only: bit-identical
 * from run to run and for every seg_rows.
 * ------------------------------------------------------------------------------------------------ */
/* bytes of `ws` for jamie_list_ranks(N, K, seg_rows): one threshold q per list entry.  0 for N < 2, K outside 1 .. 64 or a
 * seg_rows that jamie_list_ranks refuses */
long long jamie_list_ranks_workspace(long long N, int K, long long seg_rows);
/* rank[i, t] = #{ l != i : (q(i, l), l) < (q(i, j), j) }, j = idx[i, t]: idx int32 [N, K] in any order within a row, rank int32
 * [N, K], 0-based (the nearest other row has rank 0).  Row i is excluded BY INDEX; a copy of it elsewhere counts, at q = 0.  An
 * entry with j == i or j outside [0, N) gets -1 and counts nothing; a value that repeats within a row gets the same rank each
 * time.  The threshold q(i, j) of every entry is formed first, by the chain of the pair tile, into ws: both sides of every
 * comparison carry the same rounding, and integer-valued data is exact.  A NaN q (inf - inf) is read as +inf on both sides.
 * 1 <= K <= 64, 2 <= N < 2^31, L >= 1.  seg_rows: rows of X per segment of the walked side, 0 (the library's choice) or a
 * positive multiple of 128; the segments' counts are integers added into rank and the result does not depend on seg_rows.
 * Anything else, more than 65535 segments or a ws below jamie_list_ranks_workspace(N, K, seg_rows) returns an error before a
 * launch and leaves rank as it was */
int jamie_list_ranks(const float* X, long long N, int L, const int32_t* idx, int K, int32_t* rank, long long seg_rows, void* ws,
                     long long ws_bytes, void* stream);
/* The integer sums the curves are made of, from rank int32 [N, K] whose column p belongs to list position p (nearest first):
 * penalty[k - 1] = sum_i sum_{p < k} max(0, rank[i, p] + 1 - k) and overlap[k - 1] = sum_i #{ p < k : 0 <= rank[i, p] < k } for
 * k = 1 .. K (int64 [K] each), cell_penalty[i] = sum_{p < K} max(0, rank[i, p] + 1 - K) (int64 [N]).  Negative ranks count
 * nothing.  1 <= K <= 64, N >= 1 */
int jamie_coranking_sums(const int32_t* rank, long long N, int K, long long* penalty, long long* overlap, long long* cell_penalty,
                         void* stream);

/* ------------------------------------------------------------------------------------------------
 * Clustering on the device (jamie_amd/clustering.py): Lloyd's k-means of one fp32 [N, L] row-major matrix with k <= 1024 centres,
 * the two kernels of k-means++ seeding, and the contingency table of two code arrays.  q(i, j) = sum_c (X[i, c] - C[j, c])^2 as in
 * "Alignment metrics on the device": the same chain in ascending c, exact on integer-valued data.  label[i] = argmin_j by (q, then
 * lower j).  Nothing of size N x k is stored.  Deterministic: cluster sums are fp64 with one owner per (cluster, feature) element
 * and a fixed order of rows, scalars are fp64 sums in a fixed order, counts are integers; no floating-point atomics; bit-identical
 * from run to run.
 * ------------------------------------------------------------------------------------------------ */
/* bytes of `ws` for jamie_kmeans_step(N, L, k, seg_rows) (host arithmetic only): with S = ceil(N / seg_len) segments and
 * P = ceil(k L / 256): 8 S k L (the segments' fp64 tables) + 8 S (inertia) + 8 P (shift) + 4 S k (counts) + 4 S (changed labels),
 * rounded up to 16.  seg_len = seg_rows, or for seg_rows = 0 whole 128-row tiles spread evenly over at most two workgroups per
 * compute unit.  0 for arguments jamie_kmeans_step refuses */
long long jamie_kmeans_workspace(long long N, int L, int k, long long seg_rows);
/* One Lloyd iteration in one pass over X, unless state[0] (`done`) is raised: then every launch returns without touching anything.
 * state int32 [4] = {done, iterations completed, converged, reserved}, zeroed by the caller before the first iteration.
 *   assign   labels[i] (int32 [N], in place: the entry's value is the previous label) and minq[i] (fp32 [N], may be NULL) under C
 *            (fp32 [k, L]); a workgroup owns seg_len contiguous rows and walks them in 128-row tiles against centre tiles of 128
 *            with a running (q, j) minimum per row in registers
 *   sum      the rows of a tile are added into an fp64 table [k, L] in ascending row order, every element by its one owner
 *            thread; the table is in LDS while k L <= 3072, else in the segment's slab of `ws`; the segments' tables are added in
 *            segment order: sums (fp64 [k, L], may be NULL), counts (int64 [k])
 *   update   C[j] = (float)(sum[j] / count[j]) where `update` != 0; a cluster without a row keeps its centre
 *   scalars  stats (fp64 [4]) = {inertia = sum of minq (the two halves of a tile by a fixed lane tree, tiles and segments in
 *            ascending order), shift = sum ((double)C_new - (double)C_old)^2, changed labels, empty clusters}
 *   stop     state[1] += 1 = t; done is raised where (t >= 2 and no label changed) or shift <= tol_abs (both set `converged`) or
 *            t >= max_iter
 * The labels, the counts and the number of iterations do not depend on seg_rows unless two centres tie within the last bit of a
 * centre; the fp64 sums are grouped by segment, so their last bits, and through them the last bit of a centre, may.  L < 1, k
 * outside 1 .. min(N, 1024), a seg_rows that is neither 0 nor a positive multiple of 128, max_iter < 1, tol_abs < 0 or a ws below
 * jamie_kmeans_workspace(N, L, k, seg_rows) return an error before a launch */
int jamie_kmeans_step(const float* X, long long N, int L, float* C, int k, int32_t* labels, float* minq, double* sums,
                      long long* counts, double* stats, int32_t* state, double tol_abs, int max_iter, int update, long long seg_rows,
                      void* ws, long long ws_bytes, void* stream);
/* k-means++: with r = *row (a DEVICE int64, so that a pick never visits the host), minq[i] = q(X[i], X[r]) where `first` != 0, else
 * min(minq[i], q(X[i], X[r])); centre (fp32 [L], may be NULL) = X[r].  r outside [0, N) leaves everything untouched */
int jamie_kmeans_min_update(const float* X, long long N, int L, const long long* row, float* centre, float* minq, int first,
                            void* stream);
/* *pick (device int64) = the smallest i whose prefix sum of w (fp32 [N], >= 0) exceeds u * total, 0 <= u < 1, in this order of
 * additions, all in fp64: the total of every block of 1024 elements by the tree v[i] += v[i + s], s = 512, 256, ..., 1 (elements
 * past N are 0); total = the block totals added in ascending order; the block chosen is the first whose inclusive prefix of block
 * totals (ascending) exceeds u * total, the last block if none does; inside it the elements are added in ascending order onto the
 * block's exclusive prefix, and the first to exceed is picked (none by rounding: the block's last positive weight).  total == 0
 * (or NaN): pick = floor(u N).  On integer-valued w below 2^53 in total every order is exact.  ws: 8 ceil(N / 1024) bytes */
int jamie_weighted_pick(const float* w, long long N, double u, long long* pick, void* ws, long long ws_bytes, void* stream);
/* table[a[i], b[i]] += 1 for every i (a, b int32 [N]; table int64 [na, nb], integer atomics: exact).  A pair with a code outside
 * [0, na) x [0, nb) adds nothing and ORs 1 into *flag (device int32, zeroed by the caller) */
int jamie_contingency(const int32_t* a, const int32_t* b, long long N, int na, int nb, long long* table, int32_t* flag, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Layout on the device (jamie_amd/tsne.py): t-SNE of N cells into Y fp32 [N, 2] with the EXACT gradient.  The
 * affinities live on the neighbour lists of jamie_self_knn (idx int32 [N, K], dist fp32 [N, K], ascending, K <= 128), the joint
 * probabilities P in a CSR matrix of O(N K) entries, and the repulsive term is a streamed pass over all pairs of Y with per-row
 * accumulators.  Nothing of size N x N is stored.  Deterministic: no floating-point atomics, every sum has one owner and a fixed
 * order; bit-identical from run to run at the same seg_rows.
 * ------------------------------------------------------------------------------------------------ */
/* Conditional affinities, sklearn's `_binary_search_perplexity` in fp64, one wave per cell (lane l holds neighbours l and l + 64,
 * sums by a fixed xor lane tree): with e_j = d_j^2 - d_1^2 as doubles (d_1 = dist[i, 0], the nearest: s >= 1 at every beta, so no
 * cell fails), from beta = 1: P_j = exp(-beta e_j), s = sum P, H = log(s) + beta sum(e_j P_j) / s; while |H - log(perplexity)| >
 * 1e-5 and fewer than 100 tries, beta is doubled / halved until bracketed, then bisected.  C[i, slot] = (float)(P_j / s) fp32
 * [N, K], beta fp64 [N], tries int32 [N].  K outside 2 .. 128 or a perplexity outside (1, K) return an error before a launch */
int jamie_tsne_affinities(const float* dist, long long N, int K, double perplexity, float* C, double* beta, int32_t* tries,
                          void* stream);
/* For every (i, slot) with j = idx[i, slot]: mutual[i, slot] (int32) = 1 where i is in the list of j, and val[i, slot] (fp32) =
 * (float)(((double)C[i -> j] + (double)C[j -> i]) / (2 N)), a missing direction counting as 0: the joint probability of the pair,
 * the same bits from either side.  One thread per (i, slot) searching the K entries of list(j) */
int jamie_tsne_mutual(const int32_t* idx, const float* C, long long N, int K, float* val, int32_t* mutual, void* stream);
/* The CSR rows of P = (C + C^T) / (2 N) under rowptr int64 [N + 1]: row i holds its own K entries in neighbour order (col =
 * idx[i, slot], value val[i, slot]), then the cells that list i without being listed by i, in ascending index.  The latter are
 * the n_rev pairs with mutual == 0, given sorted by (target, then source): rev_pos int64 [n_rev] the flat position i K + slot of
 * the pair, rev_tgt int32 [n_rev] its target, rev_start int64 [N + 1] the exclusive prefix of the pairs per target; rowptr[i] =
 * i K + rev_start[i].  col int32 and pval fp32 have N K + n_rev entries; entries that would fall outside are not written */
int jamie_tsne_fill(const int32_t* idx, const float* val, long long N, int K, const long long* rowptr, const long long* rev_pos,
                    const int32_t* rev_tgt, const long long* rev_start, long long n_rev, int32_t* col, float* pval, void* stream);
/* bytes of `ws` for jamie_tsne_repulsion(N, seg_rows) (host arithmetic only): with S = ceil(N / seg_len) segments, 24 S N (the
 * segments' fp64 z, R_x, R_y per row) + 8 ceil(N / 256) (z per block of rows), each rounded up to 16.  seg_len = seg_rows, or for
 * seg_rows = 0 whole 128-column tiles spread evenly over S = floor(1024 / ceil(N / 1024)) segments (at least 1, at most the
 * number of tiles).  0 for arguments jamie_tsne_repulsion refuses */
long long jamie_tsne_repulsion_workspace(long long N, long long seg_rows);
/* With w_ij = 1 / (1 + |y_i - y_j|^2): R (fp64 [N, 2]) = sum over j != i of w_ij^2 (y_i - y_j), z (fp64 [N]) = sum over j != i of
 * w_ij, *Z (device fp64) = sum of z.  j = i is refused BY INDEX: a point identical to point i adds w = 1 and no force.  A workgroup
 * owns 1024 rows (four per thread, in registers) and walks one segment of the columns through LDS, 512 at a time.  fp32
 * arithmetic (w by v_rcp_f32 and one Newton step); fp32 partial sums over runs of 32 columns, each added into fp64 accumulators;
 * the segments' sums of a row are added in segment order; Z is the z of 256 rows by the tree v[t] += v[t + s], s = 128 .. 1, the
 * blocks' totals by one workgroup (thread t adds blocks t, t + 256, ..., then the same tree).  The last bits may depend on
 * seg_rows (0, or a positive multiple of 128).  Y and ws 16-byte aligned.  Anything else, more than 65535 segments or a ws below
 * jamie_tsne_repulsion_workspace(N, seg_rows) return an error before a launch */
int jamie_tsne_repulsion(const float* Y, long long N, double* R, double* z, double* Z, long long seg_rows, void* ws,
                         long long ws_bytes, void* stream);
/* bytes of `ws` for jamie_tsne_step: 16 N (a row's KL term and squared gradient) + 8 N (the gradient), each rounded up to 16 */
long long jamie_tsne_step_workspace(long long N);
/* The attractive term over the CSR rows of P (nnz entries), the gradient at Y, and (update != 0) sklearn's `_gradient_descent`
 * update of Y, u, gain (fp32 [N, 2]) in place:
 *   A_i = sum over row i of p_ij w_ij (y_i - y_j) (one wave per row: lane l takes entries l, l + 64, ... in fp32 and adds them as
 *         doubles, the lanes by a fixed xor tree; rows of any length), grad_i = (float)(4 (alpha A_i - R_i / *Z));
 *   per coordinate: gain = (u g < 0 ? gain + 0.2 : gain * 0.8), at least 0.01; u = momentum u - lr (gain g); y += u, in fp32.
 * grad (fp32 [N, 2]) and A (fp64 [N, 2]) may be NULL.  kl, gsq (device fp64, both or neither): *kl = sum over the entries of
 * p log(p (1 + d^2) *Z) and *gsq = sum of grad^2, in fp64, the rows' terms added by one workgroup in a fixed order.  Three
 * launches (attraction + gradient, the two totals when asked, the update).  An entry whose column is outside [0, N) is skipped */
int jamie_tsne_step(const long long* rowptr, const int32_t* col, const float* val, long long nnz, float* Y, long long N,
                    const double* R, const double* Z, double alpha, double momentum, double lr, float* u, float* gain, int update,
                    float* grad, double* A, double* kl, double* gsq, void* ws, long long ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * UMAP layout on the device (jamie_amd/umap.py): the fuzzy neighbour graph of N cells on the lists of
 * jamie_self_knn (idx int32 [N, K], dist fp32 [N, K], nearest first, K = n_neighbors - 1 <= 128) and the stochastic layout epochs
 * over its CSR rows (the layout of jamie_tsne_fill).  O(N K) memory.  Deterministic: no floating-point atomics; every sum and
 * every entry of the schedule has one owner; bit-identical from run to run.
 * ------------------------------------------------------------------------------------------------ */
/* Smooth kNN distances, umap-learn's `smooth_knn_dist` in fp64, one wave per cell (lane l holds neighbours l and l + 64, sums by
 * the fixed xor lane tree): rho = the smallest positive distance of the row (0 if none); psi_j(s) = exp(-(d_j - rho) / s) where
 * d_j - rho > 0, else 1; from lo = 0, hi = inf, mid = 1 and for at most 64 tries: sum = sum_j psi_j(mid); stop if |sum - target| <
 * 1e-5; if sum > target, hi = mid and mid = (lo + hi) / 2; else lo = mid and mid is doubled while hi is infinite, else (lo + hi) /
 * 2.  sigma = max(mid, 1e-3 (sum of the row's K distances) / n_neighbors).  W[i, slot] (fp32 [N, K]) = 1 where d - rho <= 0 or
 * sigma == 0, else (float)exp(-(d - rho) / sigma); rho, sigma fp64 [N]; tries int32 [N] = the sums evaluated (1 .. 64).  `target`
 * is log2(n_neighbors), passed by the caller so that both routes of jamie_amd/umap.py use one double */
int jamie_umap_smooth_knn(const float* dist, long long N, int K, int n_neighbors, double target, float* W, double* rho,
                          double* sigma, int32_t* tries, void* stream);
/* jamie_tsne_mutual with the fuzzy union: for every (i, slot) with j = idx[i, slot], mutual[i, slot] = 1 where i is in the list of
 * j, and val[i, slot] = (float)((a + b) - a b) with a = (double)W[i -> j], b = (double)W[j -> i] (0 if j does not list i): the same
 * bits from either side.  jamie_tsne_fill then writes the CSR rows */
int jamie_umap_mutual(const int32_t* idx, const float* W, long long N, int K, float* val, int32_t* mutual, void* stream);
/* One synchronous epoch `epoch` (0-based) over the CSR graph (rowptr int64 [N + 1], col int32 [nnz]; symmetric to the bit) in one
 * launch: every read of the layout is from Y_in, every write goes to Y_out (fp32 [N, 2] each, two buffers).
 *   schedule  entry e fires iff next[e] <= (float)epoch; then next[e] += eps[e] (fp32 [nnz] each; eps = +inf never fires).
 *   draws     draw r < negative_sample_rate of entry e: word r & 3 of Philox4x32-10 with counter (e & 0xffffffff, e >> 32, epoch,
 *             r >> 2) and key (seed & 0xffffffff, seed >> 32); the cell k = (word N) >> 32; k == i adds nothing.
 *   move      with d2 = fma(dx, dx, dy dy), p = powf(d2, b), q = fma(a, p, 1), clip to [-4, 4] per coordinate and coefficients
 *             0 where d2 == 0:  attraction c = ((float)(-2 a b) p) / (d2 q);  repulsion c = (float)(2 gamma b) / ((0.001 + d2) q);
 *             entry sum s = 2 clip(c_att (y_i - y_j)) + clip(c_rep (y_i - y_k0)) + clip(c_rep (y_i - y_k1)) + ... in that order;
 *             delta_i = the sum of s over the firing entries of row i;  Y_out[i] = fma((float)alpha, delta_i, Y_in[i]).
 * The factor 2 stands for the `move_other` half of entry (j, i), which fires in the same epochs.  Sixteen lanes own a row of any
 * length: lane l takes entries l, l + 16, ... in ascending order into one fp32 partial sum per coordinate, the sixteen partial
 * sums are added by the xor tree 8, 4, 2, 1, and one lane writes.  No scratch, no LDS.  delta (fp32 [N, 2]), fired (int32 [N],
 * the row's firing entries of this epoch) and fired_total (int64 [N], to which the same count is ADDED) may be NULL.  An entry
 * whose column is outside [0, N) fires but moves nothing: the entry point cannot read device memory, so `umap.epoch` and
 * `umap.optimize` check the columns of a graph once.  Y_in == Y_out, N outside [2, 2^31), a, b, gamma <= 0, alpha < 0 or a
 * negative_sample_rate outside 1 .. 64 return an error before a launch */
int jamie_umap_epoch(const long long* rowptr, const int32_t* col, const float* eps, float* next, long long nnz, const float* Y_in,
                     float* Y_out, long long N, int epoch, double alpha, double a, double b, double gamma, int negative_sample_rate,
                     unsigned long long seed, float* delta, int32_t* fired, long long* fired_total, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Spectral embedding on the device (jamie_amd/spectral.py): the products of a Chebyshev-filtered subspace
 * iteration for the leading eigenvectors of S = diag(s) A diag(s), A the CSR fuzzy graph above (rowptr int64 [N + 1], col int32,
 * val fp32 [nnz]; symmetric to the bit), s one fp64 scale per cell.  Blocks are fp64 [N, B] row-major, B = 16 or 32: a row is one
 * or two 128-byte lines.  Together they stand where umap-learn calls `umap.spectral.spectral_layout` (scipy.sparse.linalg.eigsh
 * of the normalised Laplacian) and scanpy calls `Neighbors.compute_eigen`.  O(nnz + N B) memory.  Deterministic: no atomics;
 * every sum has one owner and a fixed order; bit-identical from run to run.  1 <= N < 2^31 throughout.
 * ------------------------------------------------------------------------------------------------ */
/* out[i] = sum_j A_ij w[j] in fp64 (w == NULL: w = 1), the degree d = A 1 of `spectral_layout` / `compute_transitions`.  Sixteen
 * lanes own a row: lane l adds (double)val[e] * w[col[e]] for its entries l, l + 16, ... in ascending order (a product, then a
 * sum: no fma), the sixteen partial sums by the xor tree 8, 4, 2, 1.  An entry whose column is outside [0, N) is skipped */
int jamie_graph_rowsum(const long long* rowptr, const int32_t* col, const float* val, const double* w, long long N, long long nnz,
                       double* out, void* stream);
/* The operator apply of eigsh's matvec, one step of the three-term recurrence in one launch:
 *   out[i, l] = ((alpha scale[i]) acc + gamma in[i, l]) - beta prev[i, l],   acc = sum over the entries e of row i, ascending, of
 *   ((double)val[e] scale[col[e]]) in[col[e], l]      (every product and sum rounded on its own: no fma)
 * B lanes own a row (4 rows per wave at B = 16, 2 at B = 32) and lane l owns column l; the group loads B entries at a time, one per
 * lane, and hands (col, val scale) round by __shfl in entry order; no atomics, no LDS allocation, no scratch.  prev may
 * be NULL (the last term is then left out) and out may be prev: every element is read by its one owner before it is written.
 * out == in, prev == in, a B other than 16 or 32 or a NaN coefficient return an error before a launch.  An entry whose column
 * is outside [0, N) contributes nothing and reads nothing; `spectral.cheb_step` checks the columns of a graph once */
int jamie_graph_cheb_step(const long long* rowptr, const int32_t* col, const float* val, long long nnz, const double* scale,
                          const double* in, const double* prev, double* out, long long N, int B, double alpha, double gamma,
                          double beta, void* stream);
/* bytes of `ws` for jamie_block_gram: ceil(N / 512) B B doubles (host arithmetic; 0 for arguments it refuses) */
long long jamie_block_gram_workspace(long long N, int B);
/* out = Y^T Z, fp64 [B, B] (the Rayleigh quotient X^T S X and the Gram matrix of the orthonormalisation; LOBPCG's and ARPACK's
 * dense inner products).  Segments of 512 rows whatever the device: within a segment element (a, b) is the chain acc = fma(Y[r,
 * a], Z[r, b], acc) over the rows ascending, by one thread; the segments' sums are added in segment order by one workgroup.
 * Y == Z is allowed and gives a matrix symmetric to the bit.  `out` and `ws` differ from the blocks */
int jamie_block_gram(const double* Y, const double* Z, long long N, int B, void* ws, long long ws_bytes, double* out, void* stream);
/* out = Y1 M1 (+ Y2 M2 when both are given), M fp64 [B, B] row-major on the device: the Ritz rotation X V, the orthonormalising
 * Y (U w^-1/2) and the residual S X - X Theta.  One owner per element: a1 = fma(Y1[i, c], M1[c, l], a1) for c = 0 .. B - 1, a2
 * likewise, out = a1 + a2.  `out` differs from every input */
int jamie_block_rotate(const double* Y1, const double* M1, const double* Y2, const double* M2, long long N, int B, double* out,
                       void* stream);

/* ------------------------------------------------------------------------------------------------
 * Imputation metrics on the device (jamie_amd/imputation.py; SURVEY.md row 12, the reference's evaluation.py): per-feature
 * figures between an imputed matrix X and the measured matrix Y, both fp32 [N, d] row-major and finite.  Deterministic: fp64
 * sums in a fixed order and integer atomics only; bit-identical from run to run.
 * ------------------------------------------------------------------------------------------------ */
/* bytes of `ws` (host arithmetic only, no device needed).  which = 0: jamie_feature_stats on [N, d].  which = 1:
 * jamie_feature_auroc on a group of d features of N cells: two uint32 key buffers [d, Npad], Npad = N rounded up to a multiple of
 * 4096.  0 for any other `which` or N, d < 1 */
long long jamie_imputation_workspace(long long N, int d, int which);
/* r[f] = Pearson correlation of X[:, f] and Y[:, f], mse[f] = mean (X[:, f] - Y[:, f])^2, fp64 [d] each.  Every element is widened
 * to fp64 and shifted by row 0's value of its feature before the sums dx, dy, dx^2, dy^2, dx dy are taken in fp64; (x - y)^2 is
 * taken on the widened values.  r is NaN exactly where a column of X or of Y is constant.  2 <= N <= 65535 * 512 */
int jamie_feature_stats(const float* X, const float* Y, long long N, int d, double* r, double* mse, void* ws, long long ws_bytes,
                        void* stream);
/* For the features f in [f0, f0 + dg), 1 <= dg <= 32768: label Y[i, f] > thr[f] (strict; thr fp32 [d] on the device), score X[i, f].
 * n_pos[f] = number of positives, U2[f] = sum over the positives p of (2 #{negatives < p} + #{negatives == p}): twice the
 * Mann-Whitney U with ties at 1/2, an exact integer; AUROC = U2 / (2 n_pos n_neg).  int64 [d] each, entries outside the group
 * untouched.  Scores compare as floats (-0.0 == +0.0).  last_stage = 4; 1 .. 3 stop after the key pass, the chunk sort, the merge
 * passes (for timing the stages: U2 is then not formed) */
int jamie_feature_auroc(const float* X, const float* Y, long long N, int d, const float* thr, int f0, int dg, long long* n_pos,
                        long long* U2, void* ws, long long ws_bytes, int last_stage, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Marker features on the device (jamie_amd/markers.py; scanpy's rank_genes_groups): one-vs-rest statistics of every feature for
 * every group of cells.  X is fp32 [N, d] row-major and finite, 2 <= N <= 2^21 = 2097152: with every value of a feature tied the tie
 * term is N^3 - N, which that bound keeps below 2^63, and twice a rank stays within 32 bits.  The cells are visited in group
 * order and X is not permuted: order[N] (int32) is a stable argsort of the cells' group codes, codes[N] (int32) the codes in that
 * order (ascending, in [0, G)), seg_off[G + 1] (int32) where each group's cells start in it.  All three live on the device; an
 * entry of `order` outside [0, N) or a code outside [0, G) is skipped.  Deterministic: integer atomics and fp64 sums in a fixed
 * order only; bit-identical from run to run.
 * ------------------------------------------------------------------------------------------------ */
/* bytes of `ws` (host arithmetic only, no device needed).  which = 0: jamie_group_moments on [N, d] with G groups: fp64 partials
 * [N / 512 + G, d, 2].  which = 1: jamie_group_rank_sums on a group of d features of N cells: two uint32 key buffers [d, Npad], Npad
 * = N rounded up to a multiple of 4096.  0 for any other `which`, N, d or G < 1 or N > 2^21 */
long long jamie_markers_workspace(long long N, int d, int G, int which);
/* For the features f in [f0, f0 + dg), 1 <= dg <= 32768, with lb = #{cells j : X[j, f] < X[i, f]} and ub = #{cells j : X[j, f] <=
 * X[i, f]} of cell i: R2[f * G + g] = sum over the cells of group g of (lb + ub + 1), twice the sum of their midranks among all N
 * cells, and tie[f] = sum over all cells of ((ub - lb)^2 - 1) = sum over the tie groups of (t^3 - t).  int64, R2 [d, G] and tie [d],
 * entries outside the feature group untouched.  Values compare as floats (-0.0 == +0.0).  last_stage = 4; 1 .. 3 stop after the
 * key pass, the chunk sort, the merge passes and leave the keys in `ws` (first buffer after an even number of merge passes, else
 * the second): R2 and tie are then zero */
int jamie_group_rank_sums(const float* X, long long N, int d, const int32_t* order, const int32_t* codes, int G, int f0, int dg,
                          long long* R2, long long* tie, void* ws, long long ws_bytes, int last_stage, void* stream);
/* sums[(g * d + f) * 2 + q], fp64 [G, d, 2]: over the cells i of group g, q = 0 the sum of dx = (double)X[i, f] - (double)X[0, f],
 * q = 1 the sum of dx^2.  A group's segment is cut into pieces of 512 cells; piece_off[G + 1] (int32, device) counts the pieces of
 * the groups before each one, n_pieces = piece_off[G] <= N / 512 + G.  Within a piece cell m goes to row group m mod 16, a row group
 * adds its cells in order, the 16 row groups are added in order, and a group's pieces are added in ascending order.  d <= 65535 * 64;
 * `sums` is 16-byte aligned */
int jamie_group_moments(const float* X, long long N, int d, const int32_t* order, const int32_t* seg_off, const int32_t* piece_off,
                        int G, long long n_pieces, double* sums, void* ws, long long ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Louvain communities on the device (jamie_amd/louvain.py): one level of modularity optimisation on an integer
 * level graph of n < 2^31 nodes in CSR: rowptr[n + 1] (int64), col[nnz] (int32, never the row itself), w[nnz] (int64 >= 1),
 * loop[n] (int64 >= 0), k[n] = the row's weights + its loop, two_m = sum k < 2^52.  The state of a level is comm[n] (int32, the
 * community of every node, in [0, n)), tot[n] (int64, the k of a community's members) and size[n] (int32, their number).  All
 * arrays live on the device.  Every sum of weights is an int64 sum and the only atomics are integer ones, so every result is the
 * same bits from run to run and equals a restatement in any order.  Row extents are clamped to [0, nnz]; a column or a
 * community outside [0, n) is skipped.
 * ------------------------------------------------------------------------------------------------ */
/* w[e] = max(1, rint((double)val[e] * 2^20)) (round half to even) for the nnz entries of an fp32 CSR graph, k[i] = the sum of
 * row i's w */
int jamie_louvain_quantise(const long long* rowptr, const float* val, long long nnz, long long n, long long* w, long long* k,
                           void* stream);
/* bytes of `ws` for jamie_louvain_move on `count` rows beyond the LDS cap whose lengths are the HOST array lens[count] (host
 * arithmetic only, no device needed): 12 bytes per slot, a row of len entries owning the power of two from 2 len + 2 up.  0 for a
 * null pointer, count < 1 or a length outside [0, 2^31) */
long long jamie_louvain_workspace(const long long* lens, long long count);
/* target[i] for the nodes i of nodes[n_short + n_long + n_global] (int32, distinct), from comm, tot and size as they stand; the
 * entries of `target` of other nodes are not touched and `comm` is not written (`target` must be another array).  With c =
 * comm[i], kid = the w of row i's entries whose column is in community d, T_d = tot[d] (less k[i] for d = c):
 *     gain(d) = (double)kid - ((gamma * (double)k[i]) * (double)T_d) / (double)two_m        (fp64, this order, no contraction)
 * and target[i] is the community d of a stored neighbour with the largest gain(d) > gain(c), the lowest d among equal gains, c
 * when there is none.  When size[c] == 1 a community d > c with size[d] == 1 is not admitted.  The list holds first the n_short
 * nodes whose rows have at most 64 entries (a wave each), then the n_long ones with at most 2048 (a workgroup each, the
 * candidates in LDS), then the n_global longer ones: row r of those owns the slots [slot_off[r], slot_off[r + 1]) of `ws`
 * (slot_off int64 [n_global + 1] on the device, n_slots = slot_off[n_global], ws_bytes >= 12 n_slots, 8-byte aligned).  A node
 * whose row does not fit its part of the list, whose community is outside [0, n) or whose slots are too few keeps target = comm
 * and sets bit 0, 1 or 2 of *flag (int32 on the device, never cleared here) */
int jamie_louvain_move(const long long* rowptr, const int32_t* col, const long long* w, long long nnz, long long n,
                       const long long* k, const int32_t* comm, const long long* tot, const int32_t* size, double gamma,
                       long long two_m, const int32_t* nodes, long long n_short, long long n_long, long long n_global,
                       const long long* slot_off, long long n_slots, void* ws, long long ws_bytes, int32_t* target, int32_t* flag,
                       void* stream);
/* for the `count` distinct nodes i of `nodes` with target[i] != comm[i]: comm[i] = target[i], tot and size of the two
 * communities adjusted by k[i] and 1 (integer atomics), *moved (int64 on the device) grown by one */
int jamie_louvain_apply(const int32_t* nodes, long long count, const int32_t* target, const long long* k, int32_t* comm,
                        long long* tot, int32_t* size, long long* moved, long long n, void* stream);
/* inside[c] (int64 [n], zeroed here) = the w of the stored entries with both ends in community c, plus the loops of its nodes */
int jamie_louvain_internal(const long long* rowptr, const int32_t* col, const long long* w, long long nnz, long long n,
                           const long long* loop, const int32_t* comm, long long* inside, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Leiden communities on the device (jamie_amd/leiden.py): the refinement step of one level, on the level graph,
 * the communities comm[n] and their totals tot[n] of "Louvain communities on the device" above.  The state of a refinement is
 * ref[n] (int32, the sub-community of every node, named after its founder: a non-empty sub-community s holds node s), rtot[n]
 * (int64, the k of its members), rsize[n] (int32, their number) and cut[n] (int64, below).  Only a node that is alone (ref[i] =
 * i, rsize[i] = 1) ever moves, so a sub-community never loses a member.  With T = tot[comm[i]],
 *     wc(x, t) := (double)x >= ((gamma * (double)t) * (double)(T - t)) / (double)two_m       (fp64, this order, no contraction)
 * Every sum of weights is an int64 sum and the only atomics are integer ones: the same bits from run to run, equal to a
 * restatement in any order.  Row extents are clamped to [0, nnz]; a column or a sub-community outside [0, n) is skipped.
 * ------------------------------------------------------------------------------------------------ */
/* cut[ref[i]] += the w of row i's entries (i, j) with comm[j] = comm[i] and ref[j] != ref[i], one integer atomic per row; the
 * caller has zeroed cut[n] */
int jamie_leiden_cut(const long long* rowptr, const int32_t* col, const long long* w, long long nnz, long long n, const int32_t* comm,
                     const int32_t* ref, long long* cut, void* stream);
/* target[i] for the nodes i of nodes[n_short + n_long + n_global] (one class; the list, the three bins, slot_off, ws and *flag as
 * jamie_louvain_move), from the state as it stands; the entries of `target` of other nodes are not touched, and ref and comm are
 * not written (`target` must be another array).  A node that is no longer alone gets target[i] = ref[i] at once.  For an alone
 * node, with c = comm[i] and cut_i = the w of row i's entries inside c: target[i] = i unless wc(cut_i, k[i]); the candidates are
 * the s = ref[j] of the stored neighbours j inside c, kis = the w of row i's entries whose column is in s; s is admitted unless
 * rsize[s] = 1 and s > i, and only if wc(cut[s], rtot[s]) and
 *     gain(s) = (double)kis - ((gamma * (double)k[i]) * (double)rtot[s]) / (double)two_m > 0
 * and target[i] is the admitted s of the largest gain, the lowest s among equal gains, i when there is none */
int jamie_leiden_refine(const long long* rowptr, const int32_t* col, const long long* w, long long nnz, long long n,
                        const long long* k, const int32_t* comm, const long long* tot, const int32_t* ref, const long long* rtot,
                        const int32_t* rsize, const long long* cut, double gamma, long long two_m, const int32_t* nodes,
                        long long n_short, long long n_long, long long n_global, const long long* slot_off, long long n_slots,
                        void* ws, long long ws_bytes, int32_t* target, int32_t* flag, void* stream);
/* for the `count` distinct nodes i of `nodes` with s = target[i] != ref[i]: when target[s] != s (s's founder is itself leaving)
 * the move is cancelled and counts[1] grows by one; otherwise ref[i] = s, rtot and rsize of the two sub-communities are adjusted
 * by k[i] and 1 (integer atomics) and counts[0] grows by one.  counts is int64 [2] on the device; `target` is only read */
int jamie_leiden_apply(const int32_t* nodes, long long count, const int32_t* target, const long long* k, int32_t* ref,
                       long long* rtot, int32_t* rsize, long long* counts, long long n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Graph structure on the device (jamie_amd/graph.py): the connected components of a CSR graph of n < 2^31 nodes
 * (rowptr[n + 1] int64, col[nnz] int32; values are not read) by synchronous min-label hooking, and the kBET statistic of every
 * cell from its neighbour lists.  The state of the components is root[n] (int32: the smallest node id known for the node's tree,
 * root[root[i]] == root[i]) and the work array parent[n].  A round copies root to parent, hooks (jamie_graph_hook), then
 * compresses parent by jump passes (jamie_graph_jump, ping-pong) until a pass changes nothing: that is the next root.  The run
 * ends with the first round whose hook finds nothing; root[i] is then the smallest node id of i's component.  An entry (i, j)
 * counts when 0 <= j < n, j != i and (group == NULL or group[i] == group[j]); it links both ways whether or not its mirror is
 * stored (weak connectivity).  Duplicate entries, self loops and empty rows are legal; row extents are clamped to [0, nnz].
 * Every read of a hook comes from its input and the only atomics are integer minima, so the array after every launch is a
 * function of the launch's input: the same bits from run to run, equal to a restatement in any order.
 * ------------------------------------------------------------------------------------------------ */
/* for every entry (i, j) that counts, with a = root[i], b = root[j], a != b: parent[max(a, b)] = min(parent[max(a, b)], min(a, b))
 * (integer atomics) and *changed = 1 (int32 on the device, never cleared here).  `parent` holds a copy of `root` on entry and is
 * another array; `root` is only read.  A root outside [0, n) hooks nothing */
int jamie_graph_hook(const long long* rowptr, const int32_t* col, long long nnz, long long n, const int32_t* group,
                     const int32_t* root, int32_t* parent, int32_t* changed, void* stream);
/* out[i] = in[in[i]] for the n nodes (in[i] itself where it is outside [0, n)); *changed = 1 when some out[i] != in[i] (never
 * cleared here).  `out` is another array */
int jamie_graph_jump(const int32_t* in, int32_t* out, long long n, int32_t* changed, void* stream);
/* kBET's statistic of cell i from its K listed neighbours idx[N, K] (int32) under the categories codes[N] (int32) and the
 * expected shares expected[n_e, B] (fp64), of which the cell uses row erow[i] (row 0 when erow is NULL):
 *     o_b = #{t < K : 0 <= idx[i, t] < N and codes[idx[i, t]] == b}      (an entry or a code outside its range counts nowhere)
 *     k_i = sum_b o_b,  e_b = (double)k_i * expected[erow[i], b]
 *     stat[i] = the sum in ascending b, over the b with expected > 0, of ((o_b - e_b) * (o_b - e_b)) / e_b
 * (fp64, this order, no contraction) and df[i] = #{b : expected > 0} - 1.  When k_i = 0, df[i] < 1, a category with o_b > 0 has
 * expected 0, or erow[i] is outside [0, n_e): stat[i] = NaN and df[i] = 0 (the cell is not tested).  counts[N, B] (int32, may be
 * NULL) receives o.  1 <= K <= 128, 1 <= B <= 64 */
int jamie_kbet_stat(const int32_t* idx, long long N, int K, const int32_t* codes, int B, const double* expected, int n_e,
                    const int32_t* erow, double* stat, int32_t* df, int32_t* counts, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Sparse cell matrices (jamie_amd/sparse_input.py): `preclass(sample, axis=0)` of the reference (utilities.py:654-678; built at
 * jamie.py:462-465, applied at jamie.py:508 to the fitting sample and at jamie.py:806-837 to new cells in modal_predict /
 * transform / transform_one) for a scipy CSR matrix of N cells x d features, without a dense copy of the input on the host or the
 * device.  Stored values are fp32 (is_f64 = 0) or fp64 (is_f64 = 1); row / column pointers are int64, column indices int32, sorted
 * within a row and without duplicates.  Deterministic: fp64 partial sums per segment of 4096 stored entries of a column, added in
 * ascending order; no floating-point atomics; bit-identical from run to run.
 * ------------------------------------------------------------------------------------------------ */
/* bytes of `ws` (host arithmetic only, no device needed).  which = 0: jamie_csc_col_stats for the HOST array colptr[d + 1]: one
 * fp64 partial per segment, 8 * sum over the columns of ceil(n_c / 4096).  which = 1: jamie_csr_standardise on d features: the
 * structural-zero row, 4 d (colptr may be NULL).  0 for any other `which`, d < 1 or a decreasing colptr */
long long jamie_sparse_workspace(const long long* colptr, int d, int which);
/* mean[d], sd[d] (fp64, population standard deviation) from the nnz stored values in CSC order and colptr[d + 1] (device); row
 * indices are not needed.  With n_c stored entries in column c: mean_c = (sum of the stored v) / N and
 * sd_c = sqrt((sum of the stored (v - mean_c)^2 + (N - n_c) mean_c^2) / N), numpy's two-pass order, no term negative, divided by
 * N.  A column without stored entries gives 0 and 0, N equal stored values give that value and 0, exactly.  seg_off[d + 1] (device,
 * int64): seg_off[c] = number of segments of the columns before c, seg_off[d] = n_seg */
int jamie_csc_col_stats(const void* vals, int is_f64, long long nnz, const long long* colptr, const long long* seg_off,
                        long long n_seg, long long N, int d, double* mean, double* sd, void* ws, long long ws_bytes, void* stream);
/* out[r, c] = (float)(((double)x - mean[c]) / sd[c]), NaN -> 0, for the CSR rows r in [0, n_rows) and c in [0, d), x = 0 where
 * nothing is stored: jamie_standardise's expression, equal to it to the bit on the dense form of the same matrix.  out is fp32
 * with leading dimension ld_out >= d; columns at or beyond d are not written, every other element exactly once.  A stored column
 * index outside [0, d) is skipped, row extents are clamped to [0, nnz] */
int jamie_csr_standardise(const long long* indptr, const int32_t* indices, const void* vals, int is_f64, long long nnz,
                          long long n_rows, int d, const double* mean, const double* sd, float* out, long long ld_out, void* ws,
                          long long ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Sparse PCA products (jamie_amd/pca.py, jamie_amd/sparse_pca.py): randomized PCA of a sparse cells x features matrix X needs
 * only products with the centred matrix Xc = X - 1 mean^T, never Xc itself:
 *     Xc Q = X Q - 1 (mean^T Q),   Xc^T Y = X^T Y - mean (1^T Y),   Xc V^T = X V^T - 1 (mean^T V^T).
 * jamie_csr_spmm is the sparse x dense product with that rank-one correction in its epilogue (on the CSR arrays of X for the first
 * and third product, on the CSC arrays -- the CSR form of X^T -- for the second); jamie_weighted_colsum gives the row vector t.
 * Arrays as in "Sparse cell matrices".  Deterministic and row-local: a row's stored entries are added in stored order in fp32; a
 * row of more than 2048 entries is cut into segments of 2048 counted from its own start, each segment gives one fp32 partial [n]
 * in `ws`, and the partials are added in ascending order.  No floating-point atomics: bit-identical from run to run, and a row's
 * result is the same whether it arrives alone, in a row chunk or in the whole matrix.
 * ------------------------------------------------------------------------------------------------ */
/* bytes of `ws` for jamie_csr_spmm (host arithmetic only) from the HOST array ptr[n_rows + 1]: positions are cut into windows of
 * 2048 and every window has two partial slots of n floats, so 8 n ceil(nnz / 2048) with nnz = ptr[n_rows]; 0 when nnz <= 2048 (no
 * row can be long), for n < 1, n_rows < 1 or a decreasing ptr.  A function of nnz and n alone: jamie_csr_spmm checks it */
long long jamie_spmm_workspace(const long long* ptr, long long n_rows, int n);
/* out[r, j] = sum over the stored entries p of row r of (float)vals[p] * B[idx[p], j], minus (s ? (float)s[r] : 1) * t[j] when t
 * is given (one fused multiply-add), for r in [0, n_rows), j in [0, n).  B is fp32 [n_inner, ld_b >= n], out fp32 with leading
 * dimension ld_out >= n; fp32 accumulation, fp64 values are rounded to fp32 on load.  Columns at or beyond n of `out` are not
 * written, every other element exactly once.  A stored index outside [0, n_inner) is skipped, row extents are clamped to [0, nnz];
 * an empty row gives -s[r] t[j] */
int jamie_csr_spmm(const long long* ptr, const int32_t* idx, const void* vals, int is_f64, long long nnz, long long n_rows,
                   long long n_inner, const float* B, long long ld_b, int n, const double* s /*[n_rows] or NULL = 1*/,
                   const float* t /*[n] or NULL = no correction*/, float* out, long long ld_out, void* ws, long long ws_bytes,
                   void* stream);
/* t[j] = sum_r w[r] B[r, j] (w = NULL: ones) for the fp32 matrix B [rows, ld_b >= n]: fp64 partials per 512 rows added in ascending
 * order, rounded once to fp32.  mean^T Q with w = mean, 1^T Y with w = NULL.  ws: 8 n ceil(rows / 512) bytes, 8-byte aligned */
int jamie_weighted_colsum(const float* B, long long rows, int n, long long ld_b, const double* w /*[rows] or NULL = ones*/,
                          float* t /*[n]*/, void* ws, long long ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Feature impact on the device (jamie_amd/impact.py; build-defined): the mean squared change of the values imputed
 * for modality t when ONE input feature of modality i is replaced by a background value, per feature and target column, without
 * building the modified inputs or bringing the [features, cells, d_t] outputs to the host.  The first encoder layer is linear
 * (model.py:151), so an occluded cell's pre-activation is H + (bg_f - x_f) W0[:, f] with H = W0 x + b taken once per cell chunk.
 * Deterministic: no atomics, fixed summation order, bit-identical from run to run.
 * ------------------------------------------------------------------------------------------------ */
/* out[k n + c, m] = lrelu(bn(H[c, m] + (bg[feat[k]] - X[c, feat[k]]) * W0[m, feat[k]])) for k < g, c < n, m < h: the first hidden
 * activation of cell c with feature feat[k] occluded, in the BatchNorm-eval + LeakyReLU expression of JAMIE_EPI_BN_EVAL
 * ((v - mean) * (rsqrt(var + eps) * gamma) + beta, then v > 0 ? v : slope * v).  H [n, ldh >= h] fp32 is W0 x + b before
 * BatchNorm, X [n, ldx >= d] the cells, bg [d], W0 [h, ldw >= d] (a padded first layer: ldw > d), the four BatchNorm vectors [h],
 * out [g n, ldo >= h]; `feat` is the device copy of the host array `feat_host` [g] (unsorted, repeats allowed), which is checked
 * against [0, d) here before anything is launched: the kernels never see an unchecked index.  ws: 4 g ceil4(h) bytes on a 16-byte
 * boundary (the g columns of W0, transposed).  16-byte loads and stores when h, ldh and ldo are multiples of 4 and the pointers
 * 16-byte aligned; any h otherwise.  n <= 65535 * 32, g <= 65535, g n < 2^31 */
int jamie_occlusion_rows(const float* H, long long ldh, const float* X, long long ldx, const float* bg, const float* W0,
                         long long ldw, const int32_t* feat /*device [g]*/, const int32_t* feat_host /*host [g]*/, int n, int h, int d,
                         int g, const float* running_mean, const float* running_var, const float* gamma, const float* beta, float eps,
                         float slope, float* out, long long ldo, void* ws, long long ws_bytes, void* stream);
/* acc[k, j] += sum over c < n of ((double)Y[k n + c, j] - (double)R[c, j])^2 for k < g, j < dt: Y [g n, ldy >= dt] and
 * R [n, ldr >= dt] fp32, acc [g, dt] fp64 (contiguous).  The cells are cut into blocks of 512; a block's 16 row groups are added
 * in order, the blocks of an element in 32 interleaved slices, the slices in order, and one thread adds the total onto acc[k, j].
 * ws: 8 g dt ceil(n / 512) bytes on an 8-byte boundary.  n <= 65535 * 512, g <= 65535, g n < 2^31 */
int jamie_impact_accumulate(const float* Y, long long ldy, const float* R, long long ldr, int n, int dt, int g, double* acc, void* ws,
                            long long ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Shapley attributions on the device (jamie_amd/shapley.py; build-defined): the permutation-sampling estimator of the
 * Shapley value of F input features of modality i (the players) for the values imputed for modality t, per cell.  An order of the
 * players is walked as removals: step m sets player f_m of every cell to its background value, and the player receives the change
 * of the imputation.  The first encoder layer is linear (model.py:151), so a step changes a cell's pre-activation H = W0 x + b by
 * one rank-one term: neither the masked inputs nor the d -> 2d product per prefix exist.  Deterministic: no atomics, one owner per
 * element, fixed summation order, bit-identical from run to run.
 * ------------------------------------------------------------------------------------------------ */
/* One segment of g steps of a walk.  s_0 = state, s_m[c, :] = fmaf(-(X[c, f_m] - bg[f_m]), W0[:, f_m], s_{m-1}[c, :]) in fp32 with
 * f_m = feat[m - 1], and out[m n + c, :h] = lrelu(bn(s_m[c, :h])) for m = 0 .. g, c < n, in the BatchNorm-eval + LeakyReLU
 * expression of JAMIE_EPI_BN_EVAL ((v - mean) * (rsqrt(var + eps) * gamma) + beta, then v > 0 ? v : slope * v); on return `state`
 * holds s_g, from which the next segment of the same order continues (splitting a walk into segments changes no bit of any row).
 * state [n, lds >= h] fp32 (W0 x + b before the first segment), X [n, ldx >= d], bg [d], W0 [h, ldw >= d], the four BatchNorm
 * vectors [h], out [(g + 1) n, ldo >= h]; `feat` is the device copy of the host array `feat_host` [g], which is checked against
 * [0, d) here before anything is launched.  ws: 4 g ceil4(h) bytes on a 16-byte boundary (the g columns of W0, transposed, in walk
 * order).  16-byte loads and stores when h, lds and ldo are multiples of 4 and the pointers 16-byte aligned; any h otherwise.
 * n <= 65535 * 16, g <= 65535, (g + 1) n < 2^31 */
int jamie_shapley_walk_rows(float* state, long long lds, const float* X, long long ldx, const float* bg, const float* W0,
                            long long ldw, const int32_t* feat /*device [g]*/, const int32_t* feat_host /*host [g]*/, int n, int h,
                            int d, int g, const float* running_mean, const float* running_var, const float* gamma, const float* beta,
                            float eps, float slope, float* out, long long ldo, void* ws, long long ws_bytes, void* stream);
/* phi[c, pos[m], j] += (double)Y[m n + c, tcol[j]] - (double)Y[(m + 1) n + c, tcol[j]] for m < g, c < n, j < T: the marginal
 * contributions of one segment.  Y [(g + 1) n, ldy >= dt] fp32, phi [n, F, T] fp64 (contiguous).  pos [g]: positions in the player
 * list, distinct within a launch and in [0, F); tcol [T]: distinct columns in [0, dt), or NULL for all dt columns in order
 * (T == dt).  Both are checked here on their host copies (device copy, host copy) before anything is launched.  Every element of
 * phi has one owner per launch: no reduction, no atomics.  (g + 1) n < 2^31, n T < 2^39 */
int jamie_shapley_accumulate(const float* Y, long long ldy, int n, int dt, int g, const int32_t* pos /*device [g]*/,
                             const int32_t* pos_host /*host [g]*/, int F, const int32_t* tcol /*device [T] or NULL*/,
                             const int32_t* tcol_host /*host [T] or NULL*/, int T, double* phi, void* stream);
/* sum_abs[e] += sum over c < n of |phi[c, e]| and sum[e] += sum over c < n of phi[c, e] for e < elems: phi [n, elems] fp64
 * (contiguous), sum_abs and sum [elems] fp64.  The cells are cut into blocks of 512; a block's cells are added in order, then the
 * blocks of an element in order, and one thread adds the totals onto the outputs.  ws: 16 elems ceil(n / 512) bytes on an 8-byte
 * boundary.  n <= 65535 * 512, elems < 2^39 */
int jamie_shapley_summarise(const double* phi, int n, long long elems, double* sum_abs, double* sum, void* ws, long long ws_bytes,
                            void* stream);

/* ------------------------------------------------------------------------------------------------
 * Data-parallel exchange: RCCL collectives over xGMI behind the C ABI (`jamie_allreduce`; 8(e): cells are
 * sharded by rows over one process per GPU and the flat gradient is summed over the ranks once per step, between
 * `batch_loss.backward()` (jamie.py:734) and `clip_grad_norm_` (jamie.py:739).  The reference has no distributed code.)
 * One foreign call per collective, recordable in a launch plan like a kernel launch.  A communicator owns an RCCL communicator
 * (ncclCommInitRank on the 128-byte id rank 0 made), a HIP stream of its own and 32 completion events ("slots"): a collective
 * is enqueued on the communicator's stream BEHIND what `stream` has launched so far, so it overlaps the kernels launched after
 * it; jamie_comm_wait(slot) makes a stream wait (on the device) for the collective last issued with that slot.  librccl is
 * bound at run time (the instance already loaded in the process, else /opt/rocm/lib): a missing library is an error from these
 * entry points, not from loading libjamie_hip.so.  dtype: 0 = fp32, 1 = bf16.  Returns 1000 + ncclResult_t for an RCCL error.
 * ------------------------------------------------------------------------------------------------ */
int jamie_comm_version(int* version /*host: RCCL's NCCL_VERSION_CODE*/);
int jamie_comm_unique_id(void* id128 /*host, 128 bytes, out*/);
int jamie_comm_create(const void* id128 /*host*/, int rank, int world, void** comm /*host, out*/);
int jamie_comm_destroy(void* comm);
/* in-place SUM of buf[0 .. count) over the ranks (the 1/world average is applied inside jamie_clip_adam: hyper[13]) */
int jamie_allreduce(void* comm, void* buf, long long count, int dtype, int slot, void* stream);
/* recv[0 .. recv_count) = SUM over ranks of send[rank * recv_count .. (rank + 1) * recv_count)  (sharded optimiser: this rank's
 * piece of a large weight region's gradient) */
int jamie_reduce_scatter(void* comm, const void* send, void* recv, long long recv_count, int dtype, int slot, void* stream);
/* recv[r * send_count .. (r + 1) * send_count) = rank r's send[0 .. send_count)  (sharded optimiser: the updated weights) */
int jamie_all_gather(void* comm, const void* send, void* recv, long long send_count, int dtype, int slot, void* stream);
int jamie_comm_wait(void* comm, int slot, void* stream);

/* ------------------------------------------------------------------------------------------------
 * EXPERIMENTS (not in libjamie_hip.so; `-DJAMIE_EXPERIMENTS`, jamie_amd.build.build_experiments() -> libjamie_hip_exp.so):
 * kernels that were built, tested against the product path and measured SLOWER inside the step.  They stay as source so
 * that the measurements in profiles/ can be repeated (tests/experiments/, tools/); nothing in jamie_amd/engine.py calls them.
 * ------------------------------------------------------------------------------------------------ */
#ifdef JAMIE_EXPERIMENTS
/* Skinny products C[M, N <= 128] (fp32, written once: no slabs) = A[M, K] B[N, K]^T, both operands K-contiguous bf16, long K:
 * the heads' forward product (fc_mus | fc_vars, model.py:180,185) and the decoder-layer-0 input gradient (autograd of
 * model.py:192) on the transposed bf16 weight copy (jamie_latent_m.dec0_WT_bf16).  One workgroup per 32 x 32 output tile, its
 * 16 waves a K slice each, MFMA fragments loaded straight from global memory, partial tiles added in wave order.  Problems:
 * EPI_STORE, splitk <= 1, no transposed-operand flags; bias optional. */
int jamie_gemm_bf16_skinny(const jamie_gemm_problem* problems /*host*/, int count, void* stream);
/* Linear forward + BatchNorm1d(train) + LeakyReLU + Dropout in ONE launch (model.py:151-154 and the three sibling blocks; bf16
 * compute mode, large-tile configurations 31 / 32): jamie_gemm_bf16 on `problems` (plain stores of `splitk` fp32 slabs, bias in
 * slab 0) whose workgroups hand their slabs over INSIDE the launch -- write-through stores, one ticket per 128-column strip -- and
 * then run jamie_bn_act_fwd's strip code on `bn[i]` (whose `h`, `nslab`, `slab_stride`, `B`, `N` must describe problem i's own
 * slab buffer; `outT_bf16` must be NULL; batch <= 512, N a multiple of 4): the same bits as the two launches.
 * mode 1: the LAST workgroup of a strip to arrive reduces the whole strip; mode 2: EVERY workgroup of a strip waits (bounded) for
 * the strip's arrivals and takes a share of its eight 16-column sub-strips by arrival order (needs the strip's tiles_m x splitk
 * workgroups co-resident: they are adjacent in dispatch order).  `tickets`: device uint32 [n_tickets >= 4 + 2 * sum_i
 * ceil(N_i / 128)], zero before the first call; the launch leaves it zero; word 0 != 0 afterwards = a bounded wait gave up. */
int jamie_gemm_bf16_bn(const jamie_gemm_problem* problems /*host*/, const jamie_bnact_fwd_problem* bn /*host*/, int count /* <= 4 */,
                       int cfg, float p_drop, float momentum, float eps, float slope, const uint64_t* rng, unsigned* tickets,
                       int n_tickets, int mode, void* stream);
/* The backward products of one Linear layer -- dX = dy W on W [out, in] as stored (b_tr) and dW = dy^T a on the activations as
 * stored (a_tr + b_tr): the autograd of model.py:151,161,192,197,207 inside jamie.py:734 -- as ONE PERSISTENT launch: `n_wg`
 * workgroups (one per CU: 4 loader waves stream operands into an LDS ring by LDS-DMA, 8 consumer waves run the MFMAs and the
 * stores; hand-off through LDS words, no barrier) each work through a static list of 128 x 128 tiles.  Same arithmetic, bit for
 * bit, as jamie_gemm_bf16 on the same problems (every problem: b_tr, EPI_STORE, no bias, no accumulate; fp32 slabs, fp32 or bf16
 * (c_bf16) results, optional per-tile sums of squares in `partial`, tile id = m_tile + tiles_m * n_tile).
 *   jamie_gemm_bf16_ring_plan: the tile lists (host): sched[w * max_items + i] = (problem << 24) | tile, -1 terminated; every
 *     problem's tiles are cut into 8 contiguous chunks (workgroups w and w + 8 share an XCD) and dealt longest-first to the least
 *     loaded workgroup of the chunk's XCD.  Depends on the problems' shapes and split-K only: computed once, kept on the device.
 *   jamie_gemm_bf16_ring: the launch; `sched` is the DEVICE copy of the plan; g .. fin as in jamie_gemm_bf16_ranges (g = NULL: no
 *     range-norm riders; with riders chunk j is taken by workgroup j before its tiles); `err`: device word, zero on entry, that
 *     a hand-off poll which gave up (bounded spins; never observed) would set. */
int jamie_gemm_bf16_ring_plan(const jamie_gemm_problem* problems /*host*/, int count, int n_wg, int max_items /* <= 48 */,
                              int32_t* sched /*host, n_wg * max_items*/);
int jamie_gemm_bf16_ring(const jamie_gemm_problem* problems /*host*/, int count, const int32_t* sched /*device*/, int n_wg,
                         int max_items, const float* g, void* g_bf16, const long long* offsets /*host*/,
                         const long long* lengths /*host*/, int n_ranges, float* partials, int n_partials, uint64_t* state,
                         const jamie_latent_m* fin /*host or NULL*/, unsigned* err, void* stream);
#endif /* JAMIE_EXPERIMENTS */

#ifdef __cplusplus
}
#endif
#endif /* JAMIE_HIP_H */

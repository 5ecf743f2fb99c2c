"""ctypes binding of libjamie_hip.so (C ABI declared in include/jamie_hip.h).

There is NO CPU fallback: importing this module without the built library, or calling an op without a
GPU, raises.  PyTorch is used only for device memory and streams; every op below receives raw device
pointers and launches on torch's current HIP stream.
"""
import ctypes as C
import os

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# JAMIE_HIP_LIB: load a diagnostic build (tools/stamp_gemm_bf16.sh) instead of the in-tree product library
LIB_PATH = os.environ.get('JAMIE_HIP_LIB') or os.path.join(_HERE, 'libjamie_hip.so')

MAX_GROUP = 4
MAX_GEMM_GROUP = 8          # JAMIE_MAX_GEMM_GROUP: problems per grouped GEMM launch
MAX_GEMM_GROUP_F32 = 12     # JAMIE_MAX_GEMM_GROUP_F32: ... of the fp32 entry points
NT, NN, TN = 0, 1, 2
EPI_STORE, EPI_MSE, EPI_BN_EVAL = 0, 1, 2

c_f32p = C.c_void_p


class GemmProblem(C.Structure):
    _fields_ = [('A', C.c_void_p), ('B', C.c_void_p), ('C', C.c_void_p), ('bias', C.c_void_p),
                ('aux0', C.c_void_p), ('aux1', C.c_void_p), ('aux2', C.c_void_p), ('aux3', C.c_void_p),
                ('partial', C.c_void_p), ('a_rows', C.c_void_p),
                ('M', C.c_int), ('N', C.c_int), ('K', C.c_int),
                ('lda', C.c_int), ('ldb', C.c_int), ('ldc', C.c_int), ('aux_ld', C.c_int),
                ('splitk', C.c_int), ('slab_stride', C.c_longlong),
                ('epi', C.c_int), ('accumulate', C.c_int),
                ('scale', C.c_float), ('slope', C.c_float), ('eps', C.c_float), ('pscale', C.c_float), ('b_tr', C.c_int), ('a_tr', C.c_int), ('store_nt', C.c_int), ('c_bf16', C.c_int), ('c_panel', C.c_int)]


class CastProblem(C.Structure):
    _fields_ = [('src', C.c_void_p), ('dst', C.c_void_p), ('dstT', C.c_void_p),
                ('R', C.c_int), ('C', C.c_int), ('ld', C.c_int), ('ldd', C.c_int), ('ldt', C.c_int),
                ('nslab', C.c_int), ('slab_stride', C.c_longlong), ('src_bf16', C.c_void_p),
                ('rows', C.c_void_p), ('dst32', C.c_void_p), ('ld32', C.c_int)]


class MseProblem(C.Structure):
    _fields_ = [('y', C.c_void_p), ('x', C.c_void_p), ('d', C.c_void_p), ('d_bf16', C.c_void_p), ('dT_bf16', C.c_void_p),
                ('partial', C.c_void_p), ('R', C.c_int), ('C', C.c_int), ('nslab', C.c_int),
                ('slab_stride', C.c_longlong), ('scale', C.c_float), ('pscale', C.c_float), ('colpart', C.c_void_p)]


class ColsumProblem(C.Structure):
    _fields_ = [('X', C.c_void_p), ('out', C.c_void_p), ('M', C.c_int), ('N', C.c_int), ('ld', C.c_int),
                ('nslab', C.c_int), ('slab_stride', C.c_longlong), ('accumulate', C.c_int)]


class BnFwdProblem(C.Structure):
    _fields_ = [('h', C.c_void_p), ('nslab', C.c_int), ('slab_stride', C.c_longlong),
                ('gamma', C.c_void_p), ('beta', C.c_void_p),
                ('running_mean', C.c_void_p), ('running_var', C.c_void_p),
                ('save_mean', C.c_void_p), ('save_invstd', C.c_void_p),
                ('out', C.c_void_p), ('mask', C.c_void_p),
                ('B', C.c_int), ('N', C.c_int), ('rng_stream', C.c_int),
                ('out_bf16', C.c_void_p), ('outT_bf16', C.c_void_p), ('panel', C.c_int)]


class BnBwdProblem(C.Structure):
    _fields_ = [('da', C.c_void_p), ('nslab', C.c_int), ('slab_stride', C.c_longlong),
                ('h', C.c_void_p), ('gamma', C.c_void_p), ('beta', C.c_void_p),
                ('save_mean', C.c_void_p), ('save_invstd', C.c_void_p),
                ('dgamma', C.c_void_p), ('dbeta', C.c_void_p), ('dbias_lin', C.c_void_p),
                ('mask', C.c_void_p),
                ('B', C.c_int), ('N', C.c_int), ('rng_stream', C.c_int), ('accumulate', C.c_int),
                ('dh_bf16', C.c_void_p), ('dhT_bf16', C.c_void_p), ('skip_f32', C.c_int), ('panel', C.c_int)]


class Latent(C.Structure):
    _fields_ = [('B', C.c_int), ('L', C.c_int),
                ('ml', C.c_void_p * 2), ('ml_nslab', C.c_int), ('ml_slab_stride', C.c_longlong),
                ('head_bias', C.c_void_p * 2), ('eps_in', C.c_void_p * 2),
                ('sigma', C.c_void_p), ('corr', C.c_void_p), ('Fblk', C.c_void_p), ('hyper', C.c_void_p),
                ('mu', C.c_void_p * 2), ('lv', C.c_void_p * 2), ('z', C.c_void_p * 2),
                ('eps', C.c_void_p * 2), ('comb', C.c_void_p * 2), ('cz', C.c_void_p * 2),
                ('rsum', C.c_void_p), ('qsum', C.c_void_p), ('fc1', C.c_void_p), ('partials', C.c_void_p),
                ('dcomb', C.c_void_p * 2), ('dcomb_nslab', C.c_int), ('dcomb_slab_stride', C.c_longlong),
                ('H', C.c_void_p * 2), ('ch', C.c_void_p * 2), ('fte', C.c_void_p),
                ('dml', C.c_void_p * 2), ('dsigma', C.c_void_p),
                ('rec_partials', C.c_void_p), ('n_rec_partials', C.c_int), ('losses', C.c_void_p),
                ('cosine', C.c_int), ('rng_stream', C.c_int),
                ('dz_ext', C.c_void_p * 2), ('dmu_ext', C.c_void_p * 2), ('dlv_ext', C.c_void_p),
                ('comb_bf16', C.c_void_p * 2), ('combT_bf16', C.c_void_p * 2),
                ('dml_bf16', C.c_void_p * 2), ('dmlT_bf16', C.c_void_p * 2)]


class LatentM(C.Structure):
    _fields_ = [('B', C.c_int), ('L', C.c_int), ('M', C.c_int),
                ('ml', C.c_void_p * 4), ('ml_nslab', C.c_int), ('ml_slab_stride', C.c_longlong),
                ('head_bias', C.c_void_p * 4), ('eps_in', C.c_void_p * 4),
                ('sigma', C.c_void_p), ('hyper', C.c_void_p),
                ('mu', C.c_void_p * 4), ('lv', C.c_void_p * 4), ('z', C.c_void_p * 4), ('eps', C.c_void_p * 4),
                ('comb', C.c_void_p), ('partials', C.c_void_p),
                ('dcomb', C.c_void_p * 4), ('dcomb_nslab', C.c_int), ('dcomb_slab_stride', C.c_longlong),
                ('dml', C.c_void_p * 4), ('dsigma', C.c_void_p),
                ('rec_partials', C.c_void_p), ('n_rec_partials', C.c_int), ('losses', C.c_void_p),
                ('rng_stream', C.c_int),
                ('g1', C.c_void_p * 4), ('dec0_W', C.c_void_p * 4), ('dec0_b', C.c_void_p * 4), ('d', C.c_int * 4),
                ('comb_alias', C.c_void_p * 4), ('comb_bf16', C.c_void_p * 4), ('combT_bf16', C.c_void_p * 4),
                ('dml_bf16', C.c_void_p * 4), ('dmlT_bf16', C.c_void_p * 4),
                ('dbias_head', C.c_void_p * 4), ('colpart', C.c_void_p), ('accumulate', C.c_int), ('ticket', C.c_void_p),
                ('defer_final', C.c_int), ('head_W', C.c_void_p * 4), ('da2', C.c_void_p * 4), ('dec0_WT_bf16', C.c_void_p * 4),
                ('g1_panel', C.c_int), ('da2_panel', C.c_int)]


class SampleArgs(C.Structure):
    _fields_ = [('idx', C.c_void_p), ('B', C.c_int), ('N', C.c_longlong), ('offset', C.c_longlong), ('replace', C.c_int),
                ('rng_stream', C.c_int), ('step_add', C.c_int)]


class PdState(C.Structure):
    _fields_ = [('F', C.c_void_p), ('G1', C.c_void_p), ('G2', C.c_void_p), ('m1', C.c_void_p), ('m2', C.c_void_p),
                ('Mu', C.c_void_p), ('Lambda', C.c_void_p), ('S', C.c_void_p), ('rowsum', C.c_void_p),
                ('colsum', C.c_void_p), ('alpha', C.c_void_p), ('rowpart', C.c_void_p), ('colpart', C.c_void_p),
                ('m', C.c_int), ('n', C.c_int), ('rho', C.c_float), ('epsilon', C.c_float)]


EXPORTS = {
    'jamie_last_error': (C.c_char_p, []),
    'jamie_version': (C.c_int, []),
    'jamie_panel_width': (C.c_int, []),
    'jamie_max_partials': (C.c_int, []),
    'jamie_max_norm_partials': (C.c_int, []),
    'jamie_gemm_f32': (C.c_int, [C.POINTER(GemmProblem), C.c_int, C.c_int, C.c_void_p]),
    'jamie_gemm_f32_cfg': (C.c_int, [C.POINTER(GemmProblem), C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'jamie_gemm_tile': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'jamie_gemm_bf16': (C.c_int, [C.POINTER(GemmProblem), C.c_int, C.c_int, C.c_void_p]),
    'jamie_gemm_bf16_ranges': (C.c_int, [C.POINTER(GemmProblem), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                         C.c_void_p, C.c_int, C.c_void_p, C.POINTER(LatentM), C.c_void_p]),
    'jamie_gemm_bf16_tile': (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'jamie_comm_version': (C.c_int, [C.POINTER(C.c_int)]),
    'jamie_comm_unique_id': (C.c_int, [C.c_void_p]),
    'jamie_comm_create': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    'jamie_comm_destroy': (C.c_int, [C.c_void_p]),
    'jamie_allreduce': (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_void_p]),
    'jamie_reduce_scatter': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_void_p]),
    'jamie_all_gather': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_void_p]),
    'jamie_comm_wait': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    'jamie_cast_transpose': (C.c_int, [C.POINTER(CastProblem), C.c_int, C.c_void_p]),
    'jamie_mse_cast': (C.c_int, [C.POINTER(MseProblem), C.c_int, C.c_void_p]),
    'jamie_bn_act_fwd': (C.c_int, [C.POINTER(BnFwdProblem), C.c_int, C.c_float, C.c_float, C.c_float,
                                   C.c_float, C.c_void_p, C.c_void_p]),
    'jamie_bn_act_bwd': (C.c_int, [C.POINTER(BnBwdProblem), C.c_int, C.c_float, C.c_float, C.c_void_p,
                                   C.c_void_p]),
    'jamie_bn_act_bwd_cs': (C.c_int, [C.POINTER(BnBwdProblem), C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_int,
                                      C.c_void_p]),
    'jamie_bn_act_fwd_pf': (C.c_int, [C.POINTER(BnFwdProblem), C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    'jamie_bn_act_bwd_pf': (C.c_int, [C.POINTER(BnBwdProblem), C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_int,
                                      C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    'jamie_latent_fwd': (C.c_int, [C.POINTER(Latent), C.c_void_p, C.c_void_p]),
    'jamie_latent_bwd': (C.c_int, [C.POINTER(Latent), C.c_void_p]),
    'jamie_latent_m_fwd': (C.c_int, [C.POINTER(LatentM), C.c_void_p, C.c_void_p]),
    'jamie_latent_m_bwd': (C.c_int, [C.POINTER(LatentM), C.c_void_p]),
    'jamie_latent_m_bwd_ex': (C.c_int, [C.POINTER(LatentM), C.POINTER(SampleArgs), C.c_void_p, C.c_void_p]),
    'jamie_latent_m_colpart_size': (C.c_longlong, [C.c_int, C.c_int]),
    'jamie_optim_blocks': (C.c_int, [C.c_longlong]),
    'jamie_grad_sqnorm': (C.c_int, [C.c_void_p, C.c_longlong, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    'jamie_grad_sqnorm_bf16': (C.c_int, [C.c_void_p, C.c_longlong, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    'jamie_clip_adam_g16': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p,
                                      C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'jamie_clip_adam_ride': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p,
                                       C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(SampleArgs),
                                       C.POINTER(CastProblem), C.c_int, C.c_void_p]),
    'jamie_grad_sqnorm_ranges': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                           C.c_void_p]),
    'jamie_grad_sqnorm_ranges_g16': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                               C.c_void_p, C.c_void_p]),
    'jamie_grad_sqnorm_ranges_fin': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                               C.c_void_p, C.POINTER(LatentM), C.c_void_p, C.c_int, C.c_void_p]),
    'jamie_sqnorm_range_blocks': (C.c_int, [C.c_void_p, C.c_int]),
    'jamie_clip_adam': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p,
                                  C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'jamie_dense_block': (C.c_int, [C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_longlong,
                                    C.c_longlong, C.c_int, C.c_float, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]),
    'jamie_axpby': (C.c_int, [C.c_void_p, C.c_float, C.c_void_p, C.c_float, C.c_void_p, C.c_longlong, C.c_void_p]),
    'jamie_gather_rows': (C.c_int, [C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                    C.c_void_p]),
    'jamie_sample_indices_group': (C.c_int, [C.POINTER(SampleArgs), C.c_int, C.c_void_p, C.c_void_p]),
    'jamie_sample_indices': (C.c_int, [C.c_void_p, C.c_int, C.c_longlong, C.c_longlong, C.c_int, C.c_void_p,
                                       C.c_int, C.c_void_p]),
    'jamie_hybrid_assemble': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float,
                                        C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    'jamie_corr_from_indices': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    'jamie_csr_block': (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 5 + [C.c_void_p, C.c_void_p]),
    'jamie_colsum_group': (C.c_int, [C.POINTER(ColsumProblem), C.c_int, C.c_void_p]),
    'jamie_colsum': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_void_p,
                               C.c_int, C.c_void_p]),
    'jamie_col_stats': (C.c_int, [C.c_void_p, C.c_int, C.c_longlong, C.c_int, C.c_longlong, C.c_void_p, C.c_int,
                                  C.c_void_p, C.c_void_p, C.c_void_p]),
    'jamie_standardise': (C.c_int, [C.c_void_p, C.c_int, C.c_longlong, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p]),
    'jamie_pd_workspace': (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    'jamie_pd_step': (C.c_int, [C.POINTER(PdState), C.c_int, C.c_void_p]),
    'jamie_pd_alpha': (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_int, C.c_float, C.c_void_p,
                                 C.c_void_p]),
    'jamie_dist_workspace': (C.c_longlong, [C.c_longlong]),
    'jamie_row_sqnorm': (C.c_int, [C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p]),
    'jamie_gram_to_distances': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_void_p]),
    'jamie_row_normalise': (C.c_int, [C.c_void_p, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    'jamie_gram_to_scaled_sqdist': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_float, C.c_void_p,
                                              C.c_void_p]),
    'jamie_pairwise_absdiff': (C.c_int, [C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'jamie_knn_topk': (C.c_int, [C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p]),
    'jamie_knn_weights': (C.c_int, [C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    'jamie_knn_graph_init': (C.c_int, [C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    'jamie_apsp_fw': (C.c_int, [C.c_void_p, C.c_longlong, C.c_void_p]),
    'jamie_apsp_finalise': (C.c_int, [C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]),
    'jamie_metrics_workspace': (C.c_longlong, [C.c_longlong, C.c_longlong, C.c_int]),
    'jamie_foscttm_counts': (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_longlong, C.c_void_p]),
    'jamie_cross_knn': (C.c_int, [C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_longlong, C.c_void_p]),
    'jamie_knn_vote': (C.c_int, [C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    'jamie_label_sums_workspace': (C.c_longlong, [C.c_longlong, C.c_longlong, C.c_int, C.c_int]),
    'jamie_label_distance_sums': (C.c_int, [C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_int,
                                            C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p]),
    'jamie_silhouette_widths': (C.c_int, [C.c_void_p, C.c_longlong, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                          C.c_void_p, C.c_void_p]),
    'jamie_self_knn_workspace': (C.c_longlong, [C.c_longlong, C.c_int, C.c_longlong]),
    'jamie_self_knn': (C.c_int, [C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p,
                                 C.c_longlong, C.c_void_p]),
    'jamie_lisi': (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_void_p,
                             C.c_void_p, C.c_void_p]),
    'jamie_list_ranks_workspace': (C.c_longlong, [C.c_longlong, C.c_int, C.c_longlong]),
    'jamie_list_ranks': (C.c_int, [C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p,
                                   C.c_longlong, C.c_void_p]),
    'jamie_coranking_sums': (C.c_int, [C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'jamie_kmeans_workspace': (C.c_longlong, [C.c_longlong, C.c_int, C.c_int, C.c_longlong]),
    'jamie_kmeans_step': (C.c_int, [C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_int, C.c_longlong, C.c_void_p,
                                    C.c_longlong, C.c_void_p]),
    'jamie_kmeans_min_update': (C.c_int, [C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                          C.c_void_p]),
    'jamie_weighted_pick': (C.c_int, [C.c_void_p, C.c_longlong, C.c_double, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]),
    'jamie_contingency': (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    'jamie_tsne_affinities': (C.c_int, [C.c_void_p, C.c_longlong, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'jamie_tsne_mutual': (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    'jamie_tsne_fill': (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p]),
    'jamie_tsne_repulsion_workspace': (C.c_longlong, [C.c_longlong, C.c_longlong]),
    'jamie_tsne_repulsion': (C.c_int, [C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p,
                                       C.c_longlong, C.c_void_p]),
    'jamie_tsne_step_workspace': (C.c_longlong, [C.c_longlong]),
    'jamie_tsne_step': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p,
                                  C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]),
    'jamie_umap_smooth_knn': (C.c_int, [C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p]),
    'jamie_umap_mutual': (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    'jamie_umap_epoch': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_longlong,
                                   C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, C.c_ulonglong, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p]),
    'jamie_graph_rowsum': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_void_p,
                                     C.c_void_p]),
    'jamie_graph_cheb_step': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_longlong, C.c_int, C.c_double, C.c_double, C.c_double, C.c_void_p]),
    'jamie_block_gram_workspace': (C.c_longlong, [C.c_longlong, C.c_int]),
    'jamie_block_gram': (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]),
    'jamie_block_rotate': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p]),
    'jamie_imputation_workspace': (C.c_longlong, [C.c_longlong, C.c_int, C.c_int]),
    'jamie_feature_stats': (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong,
                                      C.c_void_p]),
    'jamie_feature_auroc': (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p]),
    'jamie_markers_workspace': (C.c_longlong, [C.c_longlong, C.c_int, C.c_int, C.c_int]),
    'jamie_group_rank_sums': (C.c_int, [C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p]),
    'jamie_group_moments': (C.c_int, [C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_longlong,
                                      C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]),
    'jamie_louvain_quantise': (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p]),
    'jamie_louvain_workspace': (C.c_longlong, [C.c_void_p, C.c_longlong]),
    'jamie_louvain_move': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_double, C.c_longlong, C.c_void_p, C.c_longlong, C.c_longlong, C.c_longlong,
                                     C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p]),
    'jamie_louvain_apply': (C.c_int, [C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_longlong, C.c_void_p]),
    'jamie_louvain_internal': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p]),
    'jamie_leiden_cut': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p]),
    'jamie_leiden_refine': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_longlong, C.c_void_p,
                                      C.c_longlong, C.c_longlong, C.c_longlong, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong,
                                      C.c_void_p, C.c_void_p, C.c_void_p]),
    'jamie_leiden_apply': (C.c_int, [C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_longlong, C.c_void_p]),
    'jamie_graph_hook': (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p]),
    'jamie_graph_jump': (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]),
    'jamie_kbet_stat': (C.c_int, [C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p]),
    'jamie_sparse_workspace': (C.c_longlong, [C.c_void_p, C.c_int, C.c_int]),
    'jamie_csc_col_stats': (C.c_int, [C.c_void_p, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_int,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]),
    'jamie_csr_standardise': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_longlong, C.c_longlong, C.c_int, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, C.c_void_p]),
    'jamie_spmm_workspace': (C.c_longlong, [C.c_void_p, C.c_longlong, C.c_int]),
    'jamie_csr_spmm': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_longlong, C.c_longlong, C.c_longlong, C.c_void_p,
                                 C.c_longlong, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong,
                                 C.c_void_p]),
    'jamie_weighted_colsum': (C.c_int, [C.c_void_p, C.c_longlong, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_longlong, C.c_void_p]),
    'jamie_occlusion_rows': (C.c_int, [C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_longlong,
                                       C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong,
                                       C.c_void_p]),
    'jamie_impact_accumulate': (C.c_int, [C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                          C.c_void_p, C.c_longlong, C.c_void_p]),
    'jamie_shapley_walk_rows': (C.c_int, [C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_longlong,
                                          C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong,
                                          C.c_void_p]),
    'jamie_shapley_accumulate': (C.c_int, [C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                           C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    'jamie_shapley_summarise': (C.c_int, [C.c_void_p, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong,
                                          C.c_void_p]),
}

# entry points of the EXPERIMENTS build only (libjamie_hip_exp.so: jamie_amd/experiments.py binds them when the loaded library has them)
EXPERIMENT_EXPORTS = {
    'jamie_gemm_bf16_ring_plan': (C.c_int, [C.POINTER(GemmProblem), C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'jamie_gemm_bf16_ring': (C.c_int, [C.POINTER(GemmProblem), C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(LatentM), C.c_void_p, C.c_void_p]),
    'jamie_gemm_bf16_skinny': (C.c_int, [C.POINTER(GemmProblem), C.c_int, C.c_void_p]),
    'jamie_gemm_bf16_bn': (C.c_int, [C.POINTER(GemmProblem), C.POINTER(BnFwdProblem), C.c_int, C.c_int, C.c_float, C.c_float,
                                     C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
}

_lib = None


class JamieHipError(RuntimeError):
    pass


def load():
    """Load the shared library (once) and declare every exported symbol's signature."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get('JAMIE_LIB') or LIB_PATH          # JAMIE_LIB: an A/B build of the same sources (tools/ab.sh)
    if not os.path.exists(path):
        raise JamieHipError(
            f'{path} is missing: build it with `python -c "import __graft_entry__ as g; g.build()"` '
            '(hipcc --offload-arch=gfx950).  jamie_amd has no CPU fallback.')
    lib = C.CDLL(path)
    for name, (res, args) in EXPORTS.items():
        fn = getattr(lib, name)          # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    for name, (res, args) in EXPERIMENT_EXPORTS.items():
        fn = getattr(lib, name, None)    # (present in an experiments build only)
        if fn is not None:
            fn.restype = res
            fn.argtypes = args
    _lib = lib
    return lib


def _check(rc):
    if rc != 0:
        raise JamieHipError(f'libjamie_hip error {rc}: {load().jamie_last_error().decode()}')


# ---------------------------------------------------------------------------------------------------
# launch plans: the training step is a fixed sequence of C-ABI calls on static buffers, so it is recorded once
# and replayed with one foreign call per launch (building the ctypes descriptors costs ~10x the call itself).
# ---------------------------------------------------------------------------------------------------
_rec = None


def begin_record():
    global _rec
    _rec = []


def end_record():
    global _rec
    plan, _rec = _rec, None
    return plan


def record_callable(fn):
    """Insert a Python callable (event record, collective, ...) into the plan being recorded; returns True if
    a recording is active (the caller should then NOT run it itself unless it wants it executed now too)."""
    if _rec is not None:
        _rec.append((fn, None))
        return True
    return False


def replay(plan):
    global _stream_override
    st = _stream()
    lib_err = None
    try:
        for fn, args in plan:
            if fn is _SET_STREAM:                # later entries launch on another HIP stream (None = torch's current)
                _stream_override = args
                st = _stream()
            elif args is None:
                fn()
            else:
                rc = fn(*args[:-1], st)          # the stream is the last argument of every launch entry point
                if rc:
                    lib_err = rc
    finally:
        _stream_override = None
    if lib_err:
        _check(lib_err)


def _call(name, *args):
    fn = getattr(load(), name)
    if _rec is not None:
        _rec.append((fn, args))
    _check(fn(*args))


# launches go to torch's current HIP stream unless `set_stream` names another one (the optimiser stream of the
# pipelined step, engine.TrainEngine.enable_pipeline); stream switches are plan entries too
_SET_STREAM = object()
_stream_override = None


def set_stream(stream):
    """Launch the following ops on `stream` (a torch.cuda.Stream; None = back to torch's current stream)."""
    global _stream_override
    _stream_override = stream
    if _rec is not None:
        _rec.append((_SET_STREAM, stream))


def current_stream():
    return _stream_override if _stream_override is not None else torch.cuda.current_stream()


def _stream():
    return C.c_void_p(current_stream().cuda_stream)


def ptr(t):
    """Device pointer of a tensor (None -> NULL).  Tensors must already live on the GPU."""
    if t is None:
        return None
    if not t.is_cuda:
        raise JamieHipError('jamie_amd ops need GPU tensors (no CPU fallback)')
    return t.data_ptr()


def require_gpu():
    if not torch.cuda.is_available():
        raise JamieHipError('no MI355X visible: jamie_amd runs on the GPU only (no CPU fallback)')
    load()


# ---------------------------------------------------------------------------------------------------
# thin op wrappers
# ---------------------------------------------------------------------------------------------------
def gemm_problem(A, B, Cout, M, N, K, lda, ldb, ldc, bias=None, splitk=1, slab_stride=0, epi=EPI_STORE,
                 accumulate=False, aux=(None, None, None, None), aux_ld=0, partial=None, a_rows=None,
                 scale=1.0, slope=0.01, eps=1e-5, pscale=1.0, b_tr=False, a_tr=False, store_nt=False, c_bf16=False, c_panel=False):
    p = GemmProblem()
    p.b_tr, p.a_tr, p.store_nt, p.c_bf16, p.c_panel = int(b_tr), int(a_tr), int(store_nt), int(c_bf16), int(c_panel)
    p.A, p.B, p.C, p.bias = ptr(A), ptr(B), ptr(Cout), ptr(bias)
    p.aux0, p.aux1, p.aux2, p.aux3 = (ptr(a) for a in aux)
    p.partial, p.a_rows = ptr(partial), ptr(a_rows)
    p.M, p.N, p.K, p.lda, p.ldb, p.ldc, p.aux_ld = M, N, K, lda, ldb, ldc, aux_ld
    p.splitk, p.slab_stride, p.epi, p.accumulate = splitk, slab_stride, epi, int(accumulate)
    p.scale, p.slope, p.eps, p.pscale = scale, slope, eps, pscale
    p._keep = (A, B, Cout, bias, aux, partial, a_rows)      # keep the tensors alive with the descriptor
    return p


def gemm(problems, layout, cfg=-1):
    arr = (GemmProblem * len(problems))(*problems)
    _call('jamie_gemm_f32_cfg', arr, len(problems), layout, cfg, _stream())


def gemm_tile(layout, max_m, max_n, max_k, cfg=-1):
    bm, bn = C.c_int(), C.c_int()
    _check(load().jamie_gemm_tile(layout, max_m, max_n, max_k, cfg, C.byref(bm), C.byref(bn)))
    return bm.value, bn.value


def gemm_bf16(problems, cfg=-1, ranges=None):
    """`ranges` = (g, g16 or None, SqRanges, partials, state, fin or None): the range-norm work (grad_sqnorm_ranges) rides as
    extra workgroups of this launch (tile configuration 29: the last dW launch of a backward pass)."""
    arr = (GemmProblem * len(problems))(*problems)
    if ranges is not None:
        g, g16, rg, partials, state, fin = ranges
        _call('jamie_gemm_bf16_ranges', arr, len(problems), cfg, ptr(g), ptr(g16), rg.off, rg.len, rg.count, ptr(partials),
              partials.numel(), ptr(state), C.pointer(fin) if fin is not None else None, _stream())
        return
    _call('jamie_gemm_bf16', arr, len(problems), cfg, _stream())


# ---- RCCL collectives behind the C ABI (csrc/comm.hip): one foreign call per collective, recordable in a launch plan ----
def _comm_dtype(t):
    if t.dtype == torch.float32:
        return 0
    if t.dtype == torch.bfloat16:
        return 1
    raise JamieHipError(f'collectives take fp32 or bf16 buffers, not {t.dtype}')


def comm_unique_id():
    """128-byte RCCL unique id (bytes): made by rank 0, handed to every rank's comm_create."""
    buf = (C.c_char * 128)()
    _check(load().jamie_comm_unique_id(buf))
    return bytes(buf)


def comm_create(uid, rank, world):
    h = C.c_void_p()
    _check(load().jamie_comm_create(C.c_char_p(uid), int(rank), int(world), C.byref(h)))
    return h


def comm_destroy(h):
    if h:
        load().jamie_comm_destroy(h)


def comm_version():
    v = C.c_int()
    _check(load().jamie_comm_version(C.byref(v)))
    return v.value


def comm_allreduce(h, buf, slot):
    _call('jamie_allreduce', h, ptr(buf), buf.numel(), _comm_dtype(buf), int(slot), _stream())


def comm_reduce_scatter(h, send, recv, slot):
    _call('jamie_reduce_scatter', h, ptr(send), ptr(recv), recv.numel(), _comm_dtype(recv), int(slot), _stream())


def comm_all_gather(h, send, recv, slot):
    _call('jamie_all_gather', h, ptr(send), ptr(recv), send.numel(), _comm_dtype(send), int(slot), _stream())


def comm_wait(h, slot):
    _call('jamie_comm_wait', h, int(slot), _stream())


def gemm_bf16_tile(max_m, max_n, cfg=-1):
    bm, bn = C.c_int(), C.c_int()
    _check(load().jamie_gemm_bf16_tile(max_m, max_n, cfg, C.byref(bm), C.byref(bn)))
    return bm.value, bn.value


def cast_problem(src, dst=None, dstT=None, nslab=1, slab_stride=0, rows=None, dst32=None):
    """fp32 [R, C] (contiguous 2-D view; slabs `slab_stride` elements apart) -> bf16 dst [R, C] / dstT [C, R].
    `rows` (int32 [R'] device tensor): output row r reads source row rows[r]; `dst32`: fp32 copy of the output rows."""
    p = CastProblem()
    R, Cc = src.shape[-2], src.shape[-1]
    if rows is not None:
        p.rows, R = ptr(rows), rows.numel()
    if dst32 is not None:
        p.dst32, p.ld32 = ptr(dst32), Cc
    if src.dtype == torch.bfloat16:      # bf16 source: transposed (or plain) copy of an existing bf16 matrix
        p.src_bf16, p.dst, p.dstT = ptr(src), ptr(dst), ptr(dstT)
    else:
        p.src, p.dst, p.dstT = ptr(src), ptr(dst), ptr(dstT)
    p.R, p.C, p.ld, p.ldd, p.ldt, p.nslab, p.slab_stride = R, Cc, Cc, Cc, R, nslab, slab_stride
    p._keep = (src, dst, dstT, rows, dst32)
    return p


def mse_problem(y, x, d, d_bf16=None, dT_bf16=None, partial=None, scale=1.0, pscale=1.0, colpart=None):
    """y [nslab, R, C] fp32 slabs (contiguous), x [R, C] fp32; outputs: d [R, C] fp32 (or None), optional bf16 [R, C] / [C, R]
    copies of d, optional `colpart` [ceil(R / 64), C] (column sums of d per 64-row tile)."""
    p = MseProblem()
    nslab = y.shape[0] if y.dim() == 3 else 1
    R, Cc = x.shape
    p.y, p.x, p.d, p.d_bf16, p.dT_bf16, p.partial = ptr(y), ptr(x), ptr(d), ptr(d_bf16), ptr(dT_bf16), ptr(partial)
    p.R, p.C, p.nslab, p.slab_stride, p.scale, p.pscale = R, Cc, nslab, R * Cc, scale, pscale
    p.colpart = ptr(colpart)
    p._keep = (y, x, d, d_bf16, dT_bf16, partial, colpart)
    return p


def mse_cast(problems):
    arr = (MseProblem * len(problems))(*problems)
    _call('jamie_mse_cast', arr, len(problems), _stream())


def cast_transpose(problems):
    for i in range(0, len(problems), 16):
        chunk = problems[i:i + 16]
        arr = (CastProblem * len(chunk))(*chunk)
        _call('jamie_cast_transpose', arr, len(chunk), _stream())


class FlatCast:
    """fp32 -> bf16 copy of a contiguous range (the data-parallel message buffer): `jamie_cast_transpose` on the range
    viewed as [R, 2048] plus a tail row; the descriptors are built once, `run(stream)` is one foreign call and is never
    recorded into a launch plan (its caller, the gradient exchange, is itself a plan entry)."""

    def __init__(self, src, dst, width=2048):
        n = src.numel()
        assert dst.numel() == n and src.dtype == torch.float32 and dst.dtype == torch.bfloat16
        probs = []
        R = n // width
        if R:
            probs.append(cast_problem(src[:R * width].view(R, width), dst[:R * width].view(R, width)))
        if n - R * width:
            probs.append(cast_problem(src[R * width:].view(1, -1), dst[R * width:].view(1, -1)))
        self.arr = (CastProblem * len(probs))(*probs)
        self.n = len(probs)
        self._keep = probs
        self.fn = load().jamie_cast_transpose

    def run(self, stream):
        _check(self.fn(self.arr, self.n, C.c_void_p(stream.cuda_stream)))


def _pf_arrays(tensors):
    """Host arrays (device pointers, byte counts rounded down to 16) of up to 8 contiguous tensors for a prefetch rider."""
    pp = (C.c_void_p * len(tensors))(*[ptr(t) for t in tensors])
    pb = (C.c_longlong * len(tensors))(*[t.numel() * t.element_size() // 16 * 16 for t in tensors])
    return pp, pb


def bn_act_fwd(problems, p_drop, rng, momentum=0.1, eps=1e-5, slope=0.01, prefetch=None):
    """`prefetch` (list of <= 8 contiguous tensors): extra workgroups read them into the caches for the next launches
    (jamie_bn_act_fwd_pf)."""
    arr = (BnFwdProblem * len(problems))(*problems)
    if prefetch:
        pp, pb = _pf_arrays(prefetch)
        arr._keep = (prefetch, pp, pb)
        _call('jamie_bn_act_fwd_pf', arr, len(problems), p_drop, momentum, eps, slope, ptr(rng), pp, pb, len(prefetch), _stream())
        return
    _call('jamie_bn_act_fwd', arr, len(problems), p_drop, momentum, eps, slope, ptr(rng), _stream())


def bn_act_bwd(problems, p_drop, rng, slope=0.01, colsums=None, prefetch=None):
    """`colsums` (from colsum_problems): column sums computed by extra workgroups of the same launch; `prefetch`: as bn_act_fwd."""
    arr = (BnBwdProblem * len(problems))(*problems)
    if prefetch:
        pp, pb = _pf_arrays(prefetch)
        arr._keep = (prefetch, pp, pb)
        _call('jamie_bn_act_bwd_pf', arr, len(problems), p_drop, slope, ptr(rng), colsums[0] if colsums is not None else None,
              colsums[1] if colsums is not None else 0, pp, pb, len(prefetch), _stream())
        return
    if colsums is not None:
        _call('jamie_bn_act_bwd_cs', arr, len(problems), p_drop, slope, ptr(rng), colsums[0], colsums[1], _stream())
        return
    _call('jamie_bn_act_bwd', arr, len(problems), p_drop, slope, ptr(rng), _stream())


def latent_fwd(desc, rng):
    _call('jamie_latent_m_fwd' if isinstance(desc, LatentM) else 'jamie_latent_fwd', C.pointer(desc), ptr(rng), _stream())


def sample_args(idx, N, offset, replace, rng_stream, step_add=0):
    """What a riding sampler draws (jamie_sample_args): idx.numel() indices of [0, N) + offset into idx."""
    a = SampleArgs()
    a.idx, a.B, a.N, a.offset, a.replace, a.rng_stream, a.step_add = ptr(idx), idx.numel(), int(N), int(offset), int(replace), \
        int(rng_stream), int(step_add)
    a._keep = idx
    return a


def latent_bwd(desc, sample=None, state=None):
    """`sample` (sample_args, fused M-modality path only): the launch's extra workgroup draws the NEXT step's batch."""
    if sample is not None:
        _call('jamie_latent_m_bwd_ex', C.pointer(desc), C.pointer(sample), ptr(state), _stream())
        return
    _call('jamie_latent_m_bwd' if isinstance(desc, LatentM) else 'jamie_latent_bwd', C.pointer(desc), _stream())


def optim_blocks(n):
    return load().jamie_optim_blocks(n)


def grad_sqnorm(g, partials, state):
    name = 'jamie_grad_sqnorm_bf16' if g.dtype == torch.bfloat16 else 'jamie_grad_sqnorm'
    _call(name, ptr(g), g.numel(), ptr(partials), partials.numel(), ptr(state), _stream())


def clip_adam(p, g, m, v, partials, hyper, state, p_bf16=None, sample=None, casts=None):
    """`g`: the fp32 gradient, or (a bf16 tensor) the reduced gradient left in its bf16 message buffer.
    Extra workgroups of the same launch, one kind at most: `sample` (sample_args) draws the next step's batch into idx;
    `casts` (list of cast_problem, <= 16) gathers / casts the next step's batch rows."""
    if sample is not None or casts:
        arr = (CastProblem * len(casts))(*casts) if casts else None
        _call('jamie_clip_adam_ride', ptr(p), ptr(g), int(g.dtype == torch.bfloat16), ptr(m), ptr(v), p.numel(), ptr(partials),
              partials.numel(), ptr(hyper), ptr(state), ptr(p_bf16), C.pointer(sample) if sample is not None else None,
              arr, len(casts) if casts else 0, _stream())
        return
    name = 'jamie_clip_adam_g16' if g.dtype == torch.bfloat16 else 'jamie_clip_adam'
    _call(name, ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), ptr(partials), partials.numel(),
          ptr(hyper), ptr(state), ptr(p_bf16), _stream())


def gather_rows(src, idx, dst):
    _call('jamie_gather_rows', ptr(src), src.shape[0], src.shape[1], ptr(idx), idx.numel(), ptr(dst), _stream())


def sample_indices_group(items, rng):
    """items = [sample_args(...)] (<= 4): independent draws in ONE launch, one workgroup each."""
    arr = (SampleArgs * len(items))(*items)
    arr._keep = items
    _call('jamie_sample_indices_group', arr, len(items), ptr(rng), _stream())


def sample_indices(idx, N, offset, replace, rng, rng_stream):
    _call('jamie_sample_indices', ptr(idx), idx.numel(), N, offset, int(replace), ptr(rng), rng_stream, _stream())


def corr_from_indices(idx0, idx1, corr):
    _call('jamie_corr_from_indices', ptr(idx0), ptr(idx1), idx0.numel(), ptr(corr), _stream())


def colsum_group(items, accumulate=False):
    """items: list of (X [M, N] contiguous fp32, out [N]) - one launch for all (bias gradients of both modalities)."""
    arr, count, _ = colsum_problems(items, accumulate)
    _call('jamie_colsum_group', arr, count, _stream())


def csr_block(indptr, indices, vals, idx0, idx1, out, row_off=0, col_off=0, normalise=True):
    """out[a, b] = P[idx0[a] + row_off, idx1[b] + col_off] for a device CSR matrix (sorted column indices)."""
    _call('jamie_csr_block', ptr(indptr), ptr(indices), ptr(vals), ptr(idx0), ptr(idx1), idx0.numel(), idx1.numel(),
          int(row_off), int(col_off), int(normalise), ptr(out), _stream())


def dense_block(Mat, idx0, idx1, out, row_off=0, col_off=0, normalise=True, w_blk=1.0, add=None, w_add=0.0):
    """out = w_blk * rownorm(Mat[idx0 + row_off][:, idx1 + col_off]) + w_add * add  (jamie.py:586-604) for a dense matrix."""
    _call('jamie_dense_block', ptr(Mat), Mat.stride(0), ptr(idx0), ptr(idx1), idx0.numel(), idx1.numel(), int(row_off),
          int(col_off), int(normalise), float(w_blk), ptr(add), float(w_add), ptr(out), _stream())


def axpby(out, a, x, b=0.0, y=None):
    _call('jamie_axpby', ptr(out), float(a), ptr(x), float(b), ptr(y), out.numel(), _stream())


def colsum(X, M, N, ld, out, nslab=1, slab_stride=0, accumulate=False):
    _call('jamie_colsum', ptr(X), M, N, ld, nslab, slab_stride, ptr(out), int(accumulate), _stream())


def pd_workspace(m, n):
    a, b = C.c_longlong(), C.c_longlong()
    _check(load().jamie_pd_workspace(m, n, C.byref(a), C.byref(b)))
    return a.value, b.value


def pd_step(state, iteration):
    _call('jamie_pd_step', C.pointer(state), int(iteration), _stream())


def pd_alpha(G2, F, partials, inv_trkk, alpha):
    _call('jamie_pd_alpha', ptr(G2), ptr(F), F.numel(), ptr(partials), partials.numel(), float(inv_trkk), ptr(alpha),
          _stream())


def standardise_columns(X):
    """Device `preclass(axis=0)`: X [N, d] fp32 / fp64 on the GPU -> (fp32 standardised [N, d], mean [d] f64, std [d] f64)."""
    if X.dtype not in (torch.float32, torch.float64) or X.dim() != 2 or not X.is_contiguous():
        raise JamieHipError('standardise_columns needs a contiguous 2-D fp32 / fp64 GPU tensor')
    N, d = X.shape
    R = int(max(1, min(256, (N + 2047) // 2048)))
    part = torch.empty(R * d, dtype=torch.float64, device=X.device)
    mean = torch.empty(d, dtype=torch.float64, device=X.device)
    sd = torch.empty(d, dtype=torch.float64, device=X.device)
    out = torch.empty(N, d, dtype=torch.float32, device=X.device)
    f64 = int(X.dtype == torch.float64)
    _call('jamie_col_stats', ptr(X), f64, N, d, d, ptr(part), R, ptr(mean), ptr(sd), _stream())
    _call('jamie_standardise', ptr(X), f64, N, d, d, ptr(mean), ptr(sd), ptr(out), _stream())
    return out, mean, sd


# ---- stage A distances (jamie_amd/distances.py; include/jamie_hip.h "Stage A distances on the device") ----
def dist_workspace(N):
    return int(load().jamie_dist_workspace(int(N)))


def row_sqnorm(X, out):
    _call('jamie_row_sqnorm', ptr(X), X.shape[0], X.shape[1], ptr(out), _stream())


def gram_to_distances(D, sqn, X, squared=False):
    """X: the [N, d] fp32 rows sqn was taken of (near-duplicate pairs are recomputed from them by direct difference)."""
    _call('jamie_gram_to_distances', ptr(D), ptr(sqn), ptr(X), D.shape[0], X.shape[1], int(squared), _stream())


def row_normalise(X, centre, out, norm):
    """X [N, d] fp32 / fp64 -> out [N, d] fp32 unit rows (row-centred first if `centre`), norm [N] fp32 (0: zero / constant row)."""
    _call('jamie_row_normalise', ptr(X), int(X.dtype == torch.float64), X.shape[0], X.shape[1], int(centre), ptr(out), ptr(norm),
          _stream())


def gram_to_scaled_sqdist(D, sqn, U, scale, rownorm):
    """U: the [N, d] fp32 (column-centred) unit rows sqn was taken of; D = scale * |u_i - u_j|^2, 1 against a row with rownorm 0."""
    _call('jamie_gram_to_scaled_sqdist', ptr(D), ptr(sqn), ptr(U), D.shape[0], U.shape[1], float(scale), ptr(rownorm), _stream())


def pairwise_absdiff(X, op, D):
    """op 0: D_ij = sum_c |x_ic - x_jc|; op 1: max_c |x_ic - x_jc|."""
    _call('jamie_pairwise_absdiff', ptr(X), X.shape[0], X.shape[1], int(op), ptr(D), _stream())


def knn_topk(D, K, idx):
    _call('jamie_knn_topk', ptr(D), D.shape[0], int(K), ptr(idx), _stream())


def knn_weights(X, idx, w):
    _call('jamie_knn_weights', ptr(X), X.shape[0], X.shape[1], ptr(idx), idx.shape[1], ptr(w), _stream())


def knn_graph_init(D, idx, w, k):
    _call('jamie_knn_graph_init', ptr(D), D.shape[0], ptr(idx), ptr(w), idx.shape[1], int(k), _stream())


def apsp_fw(D):
    _call('jamie_apsp_fw', ptr(D), D.shape[0], _stream())


def apsp_finalise(D, partials, maxv):
    _call('jamie_apsp_finalise', ptr(D), D.shape[0], ptr(partials), partials.numel(), ptr(maxv), _stream())


# ---- alignment metrics (jamie_amd/metrics.py; include/jamie_hip.h "Alignment metrics on the device") ----
def metrics_workspace(Nq, Nr, K):
    """Bytes of workspace for cross_knn(Nq, Nr, K); for foscttm_counts on N cells: (N, N, 0)."""
    return int(load().jamie_metrics_workspace(int(Nq), int(Nr), int(K)))


def foscttm_counts(A, B, row_closer, col_closer, ws):
    _call('jamie_foscttm_counts', ptr(A), ptr(B), A.shape[0], A.shape[1], ptr(row_closer), ptr(col_closer), ptr(ws),
          ws.numel() * ws.element_size(), _stream())


def cross_knn(Q, R, K, idx, dist, ws):
    _call('jamie_cross_knn', ptr(Q), Q.shape[0], ptr(R), R.shape[0], Q.shape[1], int(K), ptr(idx), ptr(dist), ptr(ws),
          ws.numel() * ws.element_size(), _stream())


def knn_vote(idx, ref_codes, n_classes, pred):
    _call('jamie_knn_vote', ptr(idx), idx.shape[0], idx.shape[1], ptr(ref_codes), int(n_classes), ptr(pred), _stream())


def label_sums_workspace(Nq, Nr, C_, seg_tiles=0):
    """Bytes of workspace for label_distance_sums of Nq queries against Nr rows in C_ classes.  Host arithmetic."""
    return int(load().jamie_label_sums_workspace(int(Nq), int(Nr), int(C_), int(seg_tiles)))


def label_distance_sums(Q, R, class_off, S, ws, seg_tiles=0):
    """S[i, c] (fp64 [Nq, >= C]) = sum of the distances of Q[i] to the rows [class_off[c], class_off[c + 1]) of R (sorted by class)."""
    _call('jamie_label_distance_sums', ptr(Q), Q.shape[0], ptr(R), R.shape[0], Q.shape[1], ptr(class_off), class_off.numel() - 1,
          ptr(S), S.stride(0), int(seg_tiles), ptr(ws), ws.numel() * ws.element_size(), _stream())


def silhouette_widths(S, counts, own, win0, wlen, out):
    _call('jamie_silhouette_widths', ptr(S), S.stride(0), S.shape[0], ptr(counts), ptr(own), ptr(win0), int(wlen), ptr(out), _stream())


# ---- neighbourhoods (jamie_amd/neighbors.py; include/jamie_hip.h "Neighbourhoods on the device") ----
def self_knn_workspace(N, K, seg_rows=0):
    """Bytes of workspace for self_knn on N rows; 0 for arguments jamie_self_knn refuses."""
    return int(load().jamie_self_knn_workspace(int(N), int(K), int(seg_rows)))


def self_knn(X, K, idx, dist, ws, seg_rows=0):
    _call('jamie_self_knn', ptr(X), X.shape[0], X.shape[1], int(K), ptr(idx), ptr(dist), int(seg_rows), ptr(ws),
          ws.numel() * ws.element_size(), _stream())


def lisi(idx, dist, codes, perplexity, out, tries=None):
    _call('jamie_lisi', ptr(idx), ptr(dist), idx.shape[0], idx.shape[1], ptr(codes), codes.shape[0], float(perplexity), ptr(out),
          ptr(tries), _stream())


# ---- layout quality (jamie_amd/coranking.py; include/jamie_hip.h "Layout quality on the device") ----
def list_ranks_workspace(N, K, seg_rows=0):
    """Bytes of workspace for list_ranks on N rows; 0 for arguments jamie_list_ranks refuses.  Host arithmetic."""
    return int(load().jamie_list_ranks_workspace(int(N), int(K), int(seg_rows)))


def list_ranks(X, idx, rank, ws, seg_rows=0):
    """rank[i, t] (int32 [N, K]) = the rows other than i that lie before row idx[i, t] in the order (q(i, .), index) of X."""
    _call('jamie_list_ranks', ptr(X), X.shape[0], X.shape[1], ptr(idx), idx.shape[1], ptr(rank), int(seg_rows), ptr(ws),
          ws.numel() * ws.element_size(), _stream())


def coranking_sums(rank, penalty, overlap, cell_penalty):
    _call('jamie_coranking_sums', ptr(rank), rank.shape[0], rank.shape[1], ptr(penalty), ptr(overlap), ptr(cell_penalty), _stream())


# ---- clustering (jamie_amd/clustering.py; include/jamie_hip.h "Clustering on the device") ----
def kmeans_workspace(N, L, k, seg_rows=0):
    """Bytes of workspace for kmeans_step; 0 for arguments jamie_kmeans_step refuses.  Host arithmetic."""
    return int(load().jamie_kmeans_workspace(int(N), int(L), int(k), int(seg_rows)))


def kmeans_step(X, C_, labels, counts, stats, state, ws, tol_abs=0.0, max_iter=1, update=True, minq=None, sums=None, seg_rows=0):
    """One Lloyd iteration under the centres C_ [k, L] (see jamie_kmeans_step); a no-op once state[0] is raised."""
    _call('jamie_kmeans_step', ptr(X), X.shape[0], X.shape[1], ptr(C_), C_.shape[0], ptr(labels), ptr(minq), ptr(sums), ptr(counts),
          ptr(stats), ptr(state), float(tol_abs), int(max_iter), int(bool(update)), int(seg_rows), ptr(ws),
          ws.numel() * ws.element_size(), _stream())


def kmeans_min_update(X, row, minq, first, centre=None):
    """minq = min(minq, q(X, X[row])) (`first`: = q) for the device int64 scalar `row`; centre [L] = X[row]."""
    _call('jamie_kmeans_min_update', ptr(X), X.shape[0], X.shape[1], ptr(row), ptr(centre), ptr(minq), int(bool(first)), _stream())


def weighted_pick(w, u, pick, ws):
    """pick (device int64 scalar) = the smallest i whose prefix sum of w exceeds u * total, in the header's order of additions."""
    _call('jamie_weighted_pick', ptr(w), w.numel(), float(u), ptr(pick), ptr(ws), ws.numel() * ws.element_size(), _stream())


def contingency(a, b, na, nb, table, flag):
    _call('jamie_contingency', ptr(a), ptr(b), a.numel(), int(na), int(nb), ptr(table), ptr(flag), _stream())


# ---- layout (jamie_amd/tsne.py; include/jamie_hip.h "Layout on the device") ----
def tsne_affinities(dist, perplexity, Cout, beta, tries):
    _call('jamie_tsne_affinities', ptr(dist), dist.shape[0], dist.shape[1], float(perplexity), ptr(Cout), ptr(beta), ptr(tries),
          _stream())


def tsne_mutual(idx, Cin, val, mutual):
    _call('jamie_tsne_mutual', ptr(idx), ptr(Cin), idx.shape[0], idx.shape[1], ptr(val), ptr(mutual), _stream())


def tsne_fill(idx, val, rowptr, rev_pos, rev_tgt, rev_start, col, pval):
    _call('jamie_tsne_fill', ptr(idx), ptr(val), idx.shape[0], idx.shape[1], ptr(rowptr), ptr(rev_pos), ptr(rev_tgt), ptr(rev_start),
          int(rev_pos.numel()), ptr(col), ptr(pval), _stream())


def tsne_repulsion_workspace(N, seg_rows=0):
    """Bytes of workspace for tsne_repulsion on N points; 0 for arguments jamie_tsne_repulsion refuses."""
    return int(load().jamie_tsne_repulsion_workspace(int(N), int(seg_rows)))


def tsne_repulsion(Y, R, z, Z, ws, seg_rows=0):
    _call('jamie_tsne_repulsion', ptr(Y), Y.shape[0], ptr(R), ptr(z), ptr(Z), int(seg_rows), ptr(ws), ws.numel(), _stream())


def tsne_step_workspace(N):
    return int(load().jamie_tsne_step_workspace(int(N)))


def tsne_step(rowptr, col, val, Y, R, Z, alpha, momentum, lr, u, gain, update, ws, grad=None, A=None, kl=None, gsq=None):
    _call('jamie_tsne_step', ptr(rowptr), ptr(col), ptr(val), int(col.numel()), ptr(Y), Y.shape[0], ptr(R), ptr(Z), float(alpha),
          float(momentum), float(lr), ptr(u), ptr(gain), int(bool(update)), ptr(grad), ptr(A), ptr(kl), ptr(gsq), ptr(ws),
          ws.numel(), _stream())


# ---- UMAP layout (jamie_amd/umap.py; include/jamie_hip.h "UMAP layout on the device") ----
def umap_smooth_knn(dist, n_neighbors, target, W, rho, sigma, tries):
    _call('jamie_umap_smooth_knn', ptr(dist), dist.shape[0], dist.shape[1], int(n_neighbors), float(target), ptr(W), ptr(rho),
          ptr(sigma), ptr(tries), _stream())


def umap_mutual(idx, W, val, mutual):
    _call('jamie_umap_mutual', ptr(idx), ptr(W), idx.shape[0], idx.shape[1], ptr(val), ptr(mutual), _stream())


def umap_epoch(rowptr, col, eps, nxt, Y_in, Y_out, epoch, alpha, a, b, gamma, negative_sample_rate, seed, delta=None, fired=None,
               fired_total=None):
    _call('jamie_umap_epoch', ptr(rowptr), ptr(col), ptr(eps), ptr(nxt), int(col.numel()), ptr(Y_in), ptr(Y_out), Y_in.shape[0],
          int(epoch), float(alpha), float(a), float(b), float(gamma), int(negative_sample_rate), int(seed) & 0xffffffffffffffff,
          ptr(delta), ptr(fired), ptr(fired_total), _stream())


# ---- spectral embedding (jamie_amd/spectral.py; include/jamie_hip.h "Spectral embedding on the device") ----
def graph_rowsum(rowptr, col, val, w, out):
    _call('jamie_graph_rowsum', ptr(rowptr), ptr(col), ptr(val), ptr(w), out.shape[0], int(col.numel()), ptr(out), _stream())


def graph_cheb_step(rowptr, col, val, scale, X, prev, out, alpha, gamma, beta):
    _call('jamie_graph_cheb_step', ptr(rowptr), ptr(col), ptr(val), int(col.numel()), ptr(scale), ptr(X), ptr(prev), ptr(out),
          X.shape[0], X.shape[1], float(alpha), float(gamma), float(beta), _stream())


def block_gram_workspace(N, B):
    """Bytes of workspace for block_gram on [N, B] blocks; 0 for arguments jamie_block_gram refuses.  Host arithmetic."""
    return int(load().jamie_block_gram_workspace(int(N), int(B)))


def block_gram(Y, Z, ws, out):
    _call('jamie_block_gram', ptr(Y), ptr(Z), Y.shape[0], Y.shape[1], ptr(ws), ws.numel() * ws.element_size(), ptr(out), _stream())


def block_rotate(Y1, M1, Y2, M2, out):
    _call('jamie_block_rotate', ptr(Y1), ptr(M1), ptr(Y2), ptr(M2), Y1.shape[0], Y1.shape[1], ptr(out), _stream())


# ---- imputation metrics (jamie_amd/imputation.py; include/jamie_hip.h "Imputation metrics on the device") ----
def imputation_workspace(N, d, which):
    """Bytes of workspace: which = 0 for feature_stats on [N, d], 1 for feature_auroc on a group of d features.  Host arithmetic."""
    return int(load().jamie_imputation_workspace(int(N), int(d), int(which)))


def feature_stats(X, Y, r, mse, ws):
    _call('jamie_feature_stats', ptr(X), ptr(Y), X.shape[0], X.shape[1], ptr(r), ptr(mse), ptr(ws), ws.numel() * ws.element_size(),
          _stream())


def feature_auroc(X, Y, thr, f0, dg, n_pos, U2, ws, last_stage=4):
    _call('jamie_feature_auroc', ptr(X), ptr(Y), X.shape[0], X.shape[1], ptr(thr), int(f0), int(dg), ptr(n_pos), ptr(U2), ptr(ws),
          ws.numel() * ws.element_size(), int(last_stage), _stream())


# ---- marker features (jamie_amd/markers.py; include/jamie_hip.h "Marker features on the device") ----
def markers_workspace(N, d, G, which):
    """Bytes of workspace: which = 0 for group_moments on [N, d] with G groups, 1 for group_rank_sums on a group of d features.
    Host arithmetic."""
    return int(load().jamie_markers_workspace(int(N), int(d), int(G), int(which)))


def group_rank_sums(X, order, codes, G, f0, dg, R2, tie, ws, last_stage=4):
    _call('jamie_group_rank_sums', ptr(X), X.shape[0], X.shape[1], ptr(order), ptr(codes), int(G), int(f0), int(dg), ptr(R2), ptr(tie),
          ptr(ws), ws.numel() * ws.element_size(), int(last_stage), _stream())


def group_moments(X, order, seg_off, piece_off, G, n_pieces, sums, ws):
    _call('jamie_group_moments', ptr(X), X.shape[0], X.shape[1], ptr(order), ptr(seg_off), ptr(piece_off), int(G), int(n_pieces),
          ptr(sums), ptr(ws), ws.numel() * ws.element_size(), _stream())


# ---- Louvain communities (jamie_amd/louvain.py; include/jamie_hip.h "Louvain communities on the device") ----
def louvain_quantise(rowptr, val, w, k):
    _call('jamie_louvain_quantise', ptr(rowptr), ptr(val), int(val.numel()), k.shape[0], ptr(w), ptr(k), _stream())


def louvain_workspace(lens):
    """Bytes of workspace for louvain_move on rows beyond the LDS cap of these lengths (a host array).  Host arithmetic."""
    lens = np.ascontiguousarray(lens, dtype=np.int64).reshape(-1)
    return int(load().jamie_louvain_workspace(lens.ctypes.data, len(lens)))


def _node_list_args(nodes, counts, slot_off, ws, target, flag):
    """The arguments louvain_move and leiden_refine end in.  `nodes`: the list from its first short row on; counts = (short, long,
    global); slot_off int64 [global + 1] or None."""
    n_slots = int(slot_off[-1].item()) if counts[2] else 0
    return (ptr(nodes), int(counts[0]), int(counts[1]), int(counts[2]), ptr(slot_off), n_slots, ptr(ws), ws.numel() * ws.element_size(),
            ptr(target), ptr(flag), _stream())


def louvain_move(rowptr, col, w, k, comm, tot, size, gamma, two_m, nodes, counts, slot_off, ws, target, flag):
    _call('jamie_louvain_move', ptr(rowptr), ptr(col), ptr(w), int(col.numel()), k.shape[0], ptr(k), ptr(comm), ptr(tot), ptr(size),
          float(gamma), int(two_m), *_node_list_args(nodes, counts, slot_off, ws, target, flag))


def louvain_apply(nodes, target, k, comm, tot, size, moved):
    _call('jamie_louvain_apply', ptr(nodes), int(nodes.numel()), ptr(target), ptr(k), ptr(comm), ptr(tot), ptr(size), ptr(moved),
          k.shape[0], _stream())


def louvain_internal(rowptr, col, w, loop, comm, inside):
    _call('jamie_louvain_internal', ptr(rowptr), ptr(col), ptr(w), int(col.numel()), loop.shape[0], ptr(loop), ptr(comm), ptr(inside),
          _stream())


# ---- Leiden communities (jamie_amd/leiden.py; include/jamie_hip.h "Leiden communities on the device") ----
def leiden_cut(rowptr, col, w, comm, ref, cut):
    """`cut` is zeroed here."""
    cut.zero_()
    _call('jamie_leiden_cut', ptr(rowptr), ptr(col), ptr(w), int(col.numel()), comm.shape[0], ptr(comm), ptr(ref), ptr(cut), _stream())


def leiden_refine(rowptr, col, w, k, comm, tot, ref, rtot, rsize, cut, gamma, two_m, nodes, counts, slot_off, ws, target, flag):
    _call('jamie_leiden_refine', ptr(rowptr), ptr(col), ptr(w), int(col.numel()), k.shape[0], ptr(k), ptr(comm), ptr(tot), ptr(ref),
          ptr(rtot), ptr(rsize), ptr(cut), float(gamma), int(two_m), *_node_list_args(nodes, counts, slot_off, ws, target, flag))


def leiden_apply(nodes, target, k, ref, rtot, rsize, counts):
    _call('jamie_leiden_apply', ptr(nodes), int(nodes.numel()), ptr(target), ptr(k), ptr(ref), ptr(rtot), ptr(rsize), ptr(counts),
          k.shape[0], _stream())


# ---- graph structure (jamie_amd/graph.py; include/jamie_hip.h "Graph structure on the device") ----
def graph_hook(rowptr, col, group, root, parent, changed):
    """`parent` holds a copy of `root`; `group` int32 [n] or None."""
    _call('jamie_graph_hook', ptr(rowptr), ptr(col), int(col.numel()), root.shape[0], ptr(group), ptr(root), ptr(parent), ptr(changed),
          _stream())


def graph_jump(src, out, changed):
    _call('jamie_graph_jump', ptr(src), ptr(out), src.shape[0], ptr(changed), _stream())


def kbet_stat(idx, codes, expected, erow, stat, df, counts=None):
    """expected float64 [n_e, B]; erow int32 [N] or None; counts int32 [N, B] or None."""
    _call('jamie_kbet_stat', ptr(idx), idx.shape[0], idx.shape[1], ptr(codes), expected.shape[1], ptr(expected), expected.shape[0],
          ptr(erow), ptr(stat), ptr(df), ptr(counts), _stream())


# ---- sparse cell matrices (jamie_amd/sparse_input.py; include/jamie_hip.h "Sparse cell matrices") ----
def sparse_workspace(colptr, d, which):
    """Bytes of workspace: which = 0 for csc_col_stats with this host `colptr` (int64 numpy [d + 1]), 1 for csr_standardise on d
    features (colptr may be None).  Host arithmetic."""
    if colptr is None:
        return int(load().jamie_sparse_workspace(None, int(d), int(which)))
    cp = np.ascontiguousarray(colptr, dtype=np.int64)
    if cp.shape != (int(d) + 1,):
        raise JamieHipError(f'sparse_workspace: colptr must have d + 1 = {int(d) + 1} entries, got shape {cp.shape}')
    return int(load().jamie_sparse_workspace(cp.ctypes.data, int(d), int(which)))


def _sparse_check(who, tensors, stats, ws):
    if any(t.dtype != torch.float64 for t in stats):
        raise JamieHipError(f'{who}: mean and sd must be float64')
    if not all(t.is_contiguous() for t in tensors):
        raise JamieHipError(f'{who}: every tensor must be contiguous')
    if ws.dtype != torch.uint8 or (ws.numel() and ws.data_ptr() % 16):
        raise JamieHipError(f'{who}: the workspace must be a uint8 tensor on a 16-byte boundary')


def csc_col_stats(vals, colptr, seg_off, n_seg, N, mean, sd, ws):
    """vals: the stored values in CSC order (fp32 / fp64), colptr / seg_off int64 [d + 1], all on the GPU; mean, sd fp64 [d]."""
    if vals.dtype not in (torch.float32, torch.float64) or colptr.dtype != torch.int64 or seg_off.dtype != torch.int64:
        raise JamieHipError('csc_col_stats needs fp32 / fp64 values and int64 colptr / seg_off')
    d = mean.numel()
    if colptr.numel() != d + 1 or seg_off.numel() != d + 1 or sd.numel() != d:
        raise JamieHipError('csc_col_stats: colptr and seg_off have d + 1 entries, mean and sd have d')
    _sparse_check('csc_col_stats', (vals, colptr, seg_off, mean, sd, ws), (mean, sd), ws)
    _call('jamie_csc_col_stats', ptr(vals) if vals.numel() else None, int(vals.dtype == torch.float64), vals.numel(), ptr(colptr),
          ptr(seg_off), int(n_seg), int(N), d, ptr(mean), ptr(sd), ptr(ws) if ws.numel() else None, ws.numel() * ws.element_size(),
          _stream())


def csr_standardise(indptr, indices, vals, d, mean, sd, out, ws, n_rows=None):
    """CSR rows [0, n_rows) (int64 indptr, int32 indices, fp32 / fp64 values, on the GPU) -> out [>= n_rows, ld_out >= d] fp32."""
    if vals.dtype not in (torch.float32, torch.float64) or indptr.dtype != torch.int64 or indices.dtype != torch.int32:
        raise JamieHipError('csr_standardise needs fp32 / fp64 values, int64 indptr and int32 indices')
    n_rows = indptr.numel() - 1 if n_rows is None else int(n_rows)
    if out.dtype != torch.float32 or out.dim() != 2 or out.stride(1) != 1 or out.shape[0] < n_rows or n_rows > indptr.numel() - 1:
        raise JamieHipError('csr_standardise: out must be fp32 [>= n_rows, >= d] with unit column stride')
    if indices.numel() != vals.numel() or mean.numel() != d or sd.numel() != d or out.shape[1] < d or out.stride(0) < out.shape[1]:
        raise JamieHipError('csr_standardise: inconsistent sizes')
    _sparse_check('csr_standardise', (indptr, indices, vals, mean, sd, ws), (mean, sd), ws)
    nnz = vals.numel()
    _call('jamie_csr_standardise', ptr(indptr), ptr(indices) if nnz else None, ptr(vals) if nnz else None,
          int(vals.dtype == torch.float64), nnz, n_rows, int(d), ptr(mean), ptr(sd), ptr(out), out.stride(0), ptr(ws),
          ws.numel() * ws.element_size(), _stream())


# ---- sparse PCA products (jamie_amd/sparse_pca.py; include/jamie_hip.h "Sparse PCA products") ----
COLSUM_ROWS = 512           # rows per fp64 partial of jamie_weighted_colsum (csrc/sparse_pca.hip: WCS_ROWS)


def spmm_workspace(indptr, n):
    """Bytes of workspace of csr_spmm with n output columns for this host `indptr` (int64 numpy [n_rows + 1]).  Host arithmetic."""
    cp = np.ascontiguousarray(indptr, dtype=np.int64)
    if cp.ndim != 1 or len(cp) < 1:
        raise JamieHipError(f'spmm_workspace: indptr must be a 1-D array, got shape {cp.shape}')
    return int(load().jamie_spmm_workspace(cp.ctypes.data, len(cp) - 1, int(n)))


def weighted_colsum_workspace(rows, n):
    return 8 * int(n) * (-(-int(rows) // COLSUM_ROWS))


def _ws_bytes(who, ws, align):
    if ws is None:
        return 0
    if ws.dtype != torch.uint8 or not ws.is_contiguous() or (ws.numel() and ws.data_ptr() % align):
        raise JamieHipError(f'{who}: the workspace must be a contiguous uint8 tensor on a {align}-byte boundary')
    return ws.numel()


def _f32_matrix(who, what, M, n):
    """ld of the fp32 matrix M [rows, >= n] with unit column stride."""
    if M.dtype != torch.float32 or M.dim() != 2:
        raise JamieHipError(f'{who}: {what} must be a 2-D float32 tensor, got {M.dtype} with {M.dim()} dimensions')
    if M.stride(1) != 1:
        raise JamieHipError(f'{who}: {what} must have unit column stride, got {M.stride(1)}')
    ld = M.stride(0) if M.shape[0] > 1 else max(M.stride(0), M.shape[1])
    if M.shape[1] < n or ld < n:
        raise JamieHipError(f'{who}: {what} has {M.shape[1]} columns with leading dimension {ld} for n = {n}')
    return ld


def csr_spmm(indptr, indices, vals, n_inner, B, out, ws=None, n=None, s=None, t=None, n_rows=None):
    """out[r, :n] = sum over the stored entries of CSR row r of value * B[index, :n], minus s[r] * t[:n] when `t` is given (s = None:
    ones).  indptr int64, indices int32, vals fp32 / fp64, B fp32 [>= n_inner, >= n], out fp32 [>= n_rows, >= n], s fp64 [n_rows],
    t fp32 [n]: GPU tensors, unit column stride.  `ws`: uint8, at least `spmm_workspace(indptr, n)` bytes (None where that is 0)."""
    who = 'csr_spmm'
    if vals.dtype not in (torch.float32, torch.float64) or indptr.dtype != torch.int64 or indices.dtype != torch.int32:
        raise JamieHipError('csr_spmm needs fp32 / fp64 values, int64 indptr and int32 indices')
    n = B.shape[1] if n is None else int(n)
    n_rows = indptr.numel() - 1 if n_rows is None else int(n_rows)
    nnz = vals.numel()
    if n < 1 or n_rows < 0 or n_rows > indptr.numel() - 1 or indices.numel() != nnz:
        raise JamieHipError(f'csr_spmm: inconsistent sizes (n = {n}, n_rows = {n_rows}, {indptr.numel()} pointers, {indices.numel()} '
                            f'indices, {nnz} values)')
    ld_b, ld_out = _f32_matrix(who, 'B', B, n), _f32_matrix(who, 'out', out, n)
    if B.shape[0] < n_inner or n_inner < 1 or out.shape[0] < n_rows:
        raise JamieHipError(f'csr_spmm: B has {B.shape[0]} rows for n_inner = {n_inner}, out {out.shape[0]} rows for n_rows = {n_rows}')
    if s is not None and (s.dtype != torch.float64 or s.numel() < n_rows or not s.is_contiguous()):
        raise JamieHipError('csr_spmm: s must be a contiguous float64 tensor of n_rows entries')
    if t is not None and (t.dtype != torch.float32 or t.numel() < n or not t.is_contiguous()):
        raise JamieHipError('csr_spmm: t must be a contiguous float32 tensor of n entries')
    if s is not None and t is None:
        raise JamieHipError('csr_spmm: s without t')
    if not all(x.is_contiguous() for x in (indptr, indices, vals)):
        raise JamieHipError('csr_spmm: the CSR arrays must be contiguous')
    have = _ws_bytes(who, ws, 4)
    need = int(load().jamie_spmm_workspace((C.c_longlong * 2)(0, nnz), 1, n))          # (a function of nnz and n alone)
    if have < need:
        raise JamieHipError(f'csr_spmm: workspace of {have} bytes, {need} needed (spmm_workspace)')
    _call('jamie_csr_spmm', ptr(indptr), ptr(indices) if nnz else None, ptr(vals) if nnz else None, int(vals.dtype == torch.float64),
          nnz, n_rows, int(n_inner), ptr(B), ld_b, n, ptr(s), ptr(t), ptr(out), ld_out, ptr(ws) if have else None, have, _stream())


def weighted_colsum(B, t, ws, w=None, n=None):
    """t[:n] = sum_r w[r] * B[r, :n] (w = None: ones) in fp64, rounded once: B fp32 [rows, >= n], w fp64 [rows], t fp32 [n];
    `ws`: uint8, `weighted_colsum_workspace(rows, n)` bytes."""
    who = 'weighted_colsum'
    n = B.shape[1] if n is None else int(n)
    if n < 1 or B.dim() != 2 or B.shape[0] < 1:
        raise JamieHipError(f'weighted_colsum: n >= 1 columns and >= 1 rows are needed, got n = {n}, B {tuple(B.shape)}')
    ld_b = _f32_matrix(who, 'B', B, n)
    rows = B.shape[0]
    if t.dtype != torch.float32 or t.numel() < n or not t.is_contiguous():
        raise JamieHipError('weighted_colsum: t must be a contiguous float32 tensor of n entries')
    if w is not None and (w.dtype != torch.float64 or w.numel() != rows or not w.is_contiguous()):
        raise JamieHipError('weighted_colsum: w must be a contiguous float64 tensor with one entry per row of B')
    have, need = _ws_bytes(who, ws, 8), weighted_colsum_workspace(rows, n)
    if have < need:
        raise JamieHipError(f'weighted_colsum: workspace of {have} bytes, {need} needed (weighted_colsum_workspace)')
    _call('jamie_weighted_colsum', ptr(B), rows, n, ld_b, ptr(w), ptr(t), ptr(ws), have, _stream())


# ---- feature impact (jamie_amd/impact.py; include/jamie_hip.h "Feature impact on the device") ----
IMPACT_ROWS = 512           # cells per fp64 partial of jamie_impact_accumulate (csrc/impact.hip: ACC_ROWS)


def occlusion_workspace(g, h):
    """Bytes of workspace of occlusion_rows for g features and h hidden units: the g columns of W0, transposed.  Host arithmetic."""
    return 4 * int(g) * ((int(h) + 3) // 4 * 4)


def impact_accumulate_workspace(n, dt, g):
    """Bytes of workspace of impact_accumulate: one fp64 partial per block of IMPACT_ROWS cells, feature and column."""
    return 8 * int(g) * int(dt) * (-(-int(n) // IMPACT_ROWS))


def check_features(feat, d, who='occlusion_rows'):
    """`feat` as a contiguous int32 numpy array [g >= 1] with every entry in [0, d), or ValueError: host arithmetic."""
    a = np.asarray(feat)
    if a.ndim != 1 or a.size < 1 or a.dtype.kind not in 'iu':
        raise ValueError(f'{who}: features must be a non-empty 1-D list of integers, got shape {a.shape} and dtype {a.dtype}')
    if int(a.min()) < 0 or int(a.max()) >= int(d):
        raise ValueError(f'{who}: feature indices must lie in [0, {int(d)}), got {int(a.min())} .. {int(a.max())}')
    return np.ascontiguousarray(a, dtype=np.int32)


def occlusion_rows(H, X, bg, W0, feat, bn, out, ws, h=None, d=None, eps=1e-5, slope=0.01, feat_dev=None):
    """out[k n + c, :h] = lrelu(bn(H[c, :h] + (bg[feat[k]] - X[c, feat[k]]) W0[:h, feat[k]])): H [n, >= h], X [n, >= d], bg [d],
    W0 [>= h, >= d], bn = (running mean, running var, gamma, beta) [>= h] each, out [g n, >= h]: fp32 GPU tensors with unit column
    stride.  `feat`: host integers [g], checked against [0, d) here; `feat_dev`: their int32 device copy where the caller keeps
    one.  `ws`: uint8, `occlusion_workspace(g, h)` bytes."""
    who = 'occlusion_rows'
    h = H.shape[1] if h is None else int(h)
    d = X.shape[1] if d is None else int(d)
    if h < 1 or d < 1 or H.dim() != 2 or H.shape[0] < 1:
        raise JamieHipError(f'occlusion_rows: n, h, d >= 1 are needed, got H {tuple(H.shape)}, h = {h}, d = {d}')
    n = H.shape[0]
    f = check_features(feat, d, who)
    g = len(f)
    ldh, ldx, ldw, ldo = _f32_matrix(who, 'H', H, h), _f32_matrix(who, 'X', X, d), _f32_matrix(who, 'W0', W0, d), _f32_matrix(who, 'out', out, h)
    if X.shape[0] != n or W0.shape[0] < h or out.shape[0] != g * n:
        raise JamieHipError(f'occlusion_rows: X has {X.shape[0]} rows for n = {n}, W0 {W0.shape[0]} for h = {h}, out {out.shape[0]} for '
                            f'g n = {g * n}')
    for t, size, what in [(bg, d, 'bg')] + [(v, h, 'a BatchNorm vector') for v in bn]:
        if t.dtype != torch.float32 or t.dim() != 1 or t.numel() < size or not t.is_contiguous():
            raise JamieHipError(f'occlusion_rows: {what} must be a contiguous float32 vector of at least {size} entries')
    if len(bn) != 4:
        raise JamieHipError('occlusion_rows: bn = (running mean, running var, gamma, beta)')
    have, need = _ws_bytes(who, ws, 16), occlusion_workspace(g, h)
    if have < need:
        raise JamieHipError(f'occlusion_rows: workspace of {have} bytes, {need} needed (occlusion_workspace)')
    if feat_dev is None:
        feat_dev = torch.from_numpy(f).to(H.device)
    elif feat_dev.dtype != torch.int32 or feat_dev.numel() != g or not feat_dev.is_contiguous():
        raise JamieHipError('occlusion_rows: feat_dev must be the contiguous int32 device copy of feat')
    _call('jamie_occlusion_rows', ptr(H), ldh, ptr(X), ldx, ptr(bg), ptr(W0), ldw, ptr(feat_dev), f.ctypes.data, n, h, d, g,
          ptr(bn[0]), ptr(bn[1]), ptr(bn[2]), ptr(bn[3]), float(eps), float(slope), ptr(out), ldo, ptr(ws), have, _stream())


def impact_accumulate(Y, R, acc, ws, dt=None):
    """acc[k, j] += sum_c (Y[k n + c, j] - R[c, j])^2 in fp64 for j < dt: Y [g n, >= dt], R [n, >= dt] fp32 with unit column stride,
    acc [g, dt] contiguous float64.  `ws`: uint8, `impact_accumulate_workspace(n, dt, g)` bytes."""
    who = 'impact_accumulate'
    dt = R.shape[1] if dt is None else int(dt)
    if dt < 1 or R.dim() != 2 or R.shape[0] < 1:
        raise JamieHipError(f'impact_accumulate: n, dt >= 1 are needed, got R {tuple(R.shape)}, dt = {dt}')
    n = R.shape[0]
    ldy, ldr = _f32_matrix(who, 'Y', Y, dt), _f32_matrix(who, 'R', R, dt)
    if acc.dtype != torch.float64 or acc.dim() != 2 or acc.shape[1] != dt or not acc.is_contiguous() or acc.shape[0] < 1:
        raise JamieHipError(f'impact_accumulate: acc must be a contiguous float64 tensor [g, {dt}], got {acc.dtype} {tuple(acc.shape)}')
    g = acc.shape[0]
    if Y.shape[0] != g * n:
        raise JamieHipError(f'impact_accumulate: Y has {Y.shape[0]} rows for g n = {g} x {n}')
    have, need = _ws_bytes(who, ws, 8), impact_accumulate_workspace(n, dt, g)
    if have < need:
        raise JamieHipError(f'impact_accumulate: workspace of {have} bytes, {need} needed (impact_accumulate_workspace)')
    _call('jamie_impact_accumulate', ptr(Y), ldy, ptr(R), ldr, n, dt, g, ptr(acc), ptr(ws), have, _stream())


# ---- Shapley attributions (jamie_amd/shapley.py; include/jamie_hip.h "Shapley attributions on the device") ----
SHAPLEY_ROWS = 512          # cells per fp64 partial of jamie_shapley_summarise (csrc/shapley.hip: SUM_ROWS)


def shapley_walk_workspace(g, h):
    """Bytes of workspace of shapley_walk_rows for g steps and h hidden units: the g columns of W0, transposed.  Host arithmetic."""
    return 4 * int(g) * ((int(h) + 3) // 4 * 4)


def shapley_summarise_workspace(n, elems):
    """Bytes of workspace of shapley_summarise: two fp64 partials per block of SHAPLEY_ROWS cells and element."""
    return 16 * int(elems) * (-(-int(n) // SHAPLEY_ROWS))


def check_distinct(idx, bound, who, what):
    """`idx` as a contiguous int32 numpy array [>= 1] of DISTINCT entries in [0, bound), or ValueError: host arithmetic."""
    a = check_features(idx, bound, who)
    if len(np.unique(a)) != len(a):
        raise ValueError(f'{who}: {what} must be distinct, got {len(a) - len(np.unique(a))} repeated among {len(a)}')
    return a


def _device_copy(who, what, host, dev, like):
    if dev is None:
        return torch.from_numpy(host).to(like.device)
    if dev.dtype != torch.int32 or dev.numel() != len(host) or not dev.is_contiguous():
        raise JamieHipError(f'{who}: {what} must be the contiguous int32 device copy of its host array')
    return dev


def shapley_walk_rows(state, X, bg, W0, feat, bn, out, ws, h=None, d=None, eps=1e-5, slope=0.01, feat_dev=None):
    """One segment of a walk: s_0 = state, s_m = fmaf(-(X[:, feat[m - 1]] - bg[feat[m - 1]]), W0[:h, feat[m - 1]], s_{m - 1}),
    out[m n + c, :h] = lrelu(bn(s_m[c, :h])) for m = 0 .. g, and state = s_g on return.  state [n, >= h] (read and written),
    X [n, >= d], bg [d], W0 [>= h, >= d], bn = (running mean, running var, gamma, beta) [>= h] each, out [(g + 1) n, >= h]: fp32 GPU
    tensors with unit column stride.  `feat`: host integers [g], checked against [0, d) here; `feat_dev`: their int32 device copy
    where the caller keeps one.  `ws`: uint8, `shapley_walk_workspace(g, h)` bytes."""
    who = 'shapley_walk_rows'
    h = state.shape[1] if h is None else int(h)
    d = X.shape[1] if d is None else int(d)
    if h < 1 or d < 1 or state.dim() != 2 or state.shape[0] < 1:
        raise JamieHipError(f'{who}: n, h, d >= 1 are needed, got state {tuple(state.shape)}, h = {h}, d = {d}')
    n = state.shape[0]
    f = check_features(feat, d, who)
    g = len(f)
    lds, ldx, ldw, ldo = (_f32_matrix(who, 'state', state, h), _f32_matrix(who, 'X', X, d), _f32_matrix(who, 'W0', W0, d),
                          _f32_matrix(who, 'out', out, h))
    if X.shape[0] != n or W0.shape[0] < h or out.shape[0] != (g + 1) * n:
        raise JamieHipError(f'{who}: X has {X.shape[0]} rows for n = {n}, W0 {W0.shape[0]} for h = {h}, out {out.shape[0]} for '
                            f'(g + 1) n = {(g + 1) * n}')
    if len(bn) != 4:
        raise JamieHipError(f'{who}: bn = (running mean, running var, gamma, beta)')
    for t, size, what in [(bg, d, 'bg')] + [(v, h, 'a BatchNorm vector') for v in bn]:
        if t.dtype != torch.float32 or t.dim() != 1 or t.numel() < size or not t.is_contiguous():
            raise JamieHipError(f'{who}: {what} must be a contiguous float32 vector of at least {size} entries')
    have, need = _ws_bytes(who, ws, 16), shapley_walk_workspace(g, h)
    if have < need:
        raise JamieHipError(f'{who}: workspace of {have} bytes, {need} needed (shapley_walk_workspace)')
    feat_dev = _device_copy(who, 'feat_dev', f, feat_dev, state)
    _call('jamie_shapley_walk_rows', ptr(state), lds, ptr(X), ldx, ptr(bg), ptr(W0), ldw, ptr(feat_dev), f.ctypes.data, n, h, d, g,
          ptr(bn[0]), ptr(bn[1]), ptr(bn[2]), ptr(bn[3]), float(eps), float(slope), ptr(out), ldo, ptr(ws), have, _stream())


def shapley_accumulate(Y, pos, phi, tcol=None, dt=None, pos_dev=None, tcol_dev=None):
    """phi[c, pos[m], j] += (double)Y[m n + c, tcol[j]] - (double)Y[(m + 1) n + c, tcol[j]]: Y [(g + 1) n, >= dt] fp32 with unit
    column stride, phi [n, F, T] contiguous float64, `pos` host integers [g], distinct and in [0, F), `tcol` host integers [T],
    distinct and in [0, dt), or None for all dt columns in order (T == dt).  `pos_dev`, `tcol_dev`: their int32 device copies
    where the caller keeps them."""
    who = 'shapley_accumulate'
    dt = Y.shape[1] if dt is None else int(dt)
    if phi.dtype != torch.float64 or phi.dim() != 3 or not phi.is_contiguous() or min(phi.shape) < 1:
        raise JamieHipError(f'{who}: phi must be a contiguous float64 tensor [n, F, T], got {phi.dtype} {tuple(phi.shape)}')
    n, F, T = phi.shape
    if dt < 1:
        raise JamieHipError(f'{who}: dt >= 1 is needed, got {dt}')
    ldy = _f32_matrix(who, 'Y', Y, dt)
    p = check_distinct(pos, F, who, 'the positions')
    g = len(p)
    if Y.shape[0] != (g + 1) * n:
        raise JamieHipError(f'{who}: Y has {Y.shape[0]} rows for (g + 1) n = {g + 1} x {n}')
    tc = None if tcol is None else check_distinct(tcol, dt, who, 'the target columns')
    if (T != dt) if tc is None else (len(tc) != T):
        raise JamieHipError(f'{who}: phi has {T} target columns for {dt if tc is None else len(tc)} requested')
    pos_dev = _device_copy(who, 'pos_dev', p, pos_dev, Y)
    tcol_dev = None if tc is None else _device_copy(who, 'tcol_dev', tc, tcol_dev, Y)
    _call('jamie_shapley_accumulate', ptr(Y), ldy, n, dt, g, ptr(pos_dev), p.ctypes.data, F, ptr(tcol_dev),
          None if tc is None else tc.ctypes.data, T, ptr(phi), _stream())


def shapley_summarise(phi, sum_abs, total, ws):
    """sum_abs[e] += sum_c |phi[c, e]| and total[e] += sum_c phi[c, e] over the leading dimension of the contiguous float64 tensor
    `phi` [n, ...]; sum_abs and total: contiguous float64 with phi[0].numel() entries.  `ws`: uint8,
    `shapley_summarise_workspace(n, elems)` bytes."""
    who = 'shapley_summarise'
    if phi.dtype != torch.float64 or phi.dim() < 2 or not phi.is_contiguous() or phi.numel() < 1:
        raise JamieHipError(f'{who}: phi must be a non-empty contiguous float64 tensor [n, ...], got {phi.dtype} {tuple(phi.shape)}')
    n, elems = phi.shape[0], phi[0].numel()
    for t, what in ((sum_abs, 'sum_abs'), (total, 'total')):
        if t.dtype != torch.float64 or t.numel() != elems or not t.is_contiguous():
            raise JamieHipError(f'{who}: {what} must be a contiguous float64 tensor of {elems} entries, got {t.dtype} {tuple(t.shape)}')
    have, need = _ws_bytes(who, ws, 8), shapley_summarise_workspace(n, elems)
    if have < need:
        raise JamieHipError(f'{who}: workspace of {have} bytes, {need} needed (shapley_summarise_workspace)')
    _call('jamie_shapley_summarise', ptr(phi), n, elems, ptr(sum_abs), ptr(total), ptr(ws), have, _stream())


class SqRanges:
    """Host description of the gradient ranges jamie_grad_sqnorm_ranges covers (kept alive for recorded plans)."""

    def __init__(self, ranges):
        self.count = len(ranges)
        self.off = (C.c_longlong * self.count)(*[int(a) for a, _ in ranges])
        self.len = (C.c_longlong * self.count)(*[int(b) for _, b in ranges])
        self.blocks = load().jamie_sqnorm_range_blocks(self.len, self.count)


def colsum_problems(items, accumulate=False):
    """[(X [M, N] contiguous fp32, out [N])] -> (ctypes array, count, partial slots: ceil(N / 64) each)."""
    probs = []
    for X, out in items:
        p = ColsumProblem()
        p.X, p.out, p.M, p.N, p.ld, p.nslab, p.slab_stride, p.accumulate = ptr(X), ptr(out), X.shape[0], X.shape[1], X.shape[1], 1, 0, int(accumulate)
        probs.append(p)
    arr = (ColsumProblem * len(probs))(*probs)
    arr._keep = items
    return arr, len(probs), sum((X.shape[1] + 63) // 64 for X, _ in items)


def grad_sqnorm_ranges(g, ranges, partials, state, g16=None, fin=None, colsums=None):
    """`g16` (flat bf16, same layout as g): also receives the bf16 copy of every range.  `fin` (a LatentM with defer_final):
    one extra workgroup finalises the latent backward pass; `colsums` (from colsum_problems): further extra workgroups write
    column sums into g; `partials` has one more slot per extra workgroup."""
    if fin is not None:
        arr, cnt = (colsums[0], colsums[1]) if colsums is not None else (None, 0)
        _call('jamie_grad_sqnorm_ranges_fin', ptr(g), ptr(g16), ranges.off, ranges.len, ranges.count, ptr(partials),
              partials.numel(), ptr(state), C.pointer(fin), arr, cnt, _stream())
        return
    if g16 is not None:
        _call('jamie_grad_sqnorm_ranges_g16', ptr(g), ptr(g16), ranges.off, ranges.len, ranges.count, ptr(partials),
              partials.numel(), ptr(state), _stream())
        return
    _call('jamie_grad_sqnorm_ranges', ptr(g), ranges.off, ranges.len, ranges.count, ptr(partials), partials.numel(),
          ptr(state), _stream())


def hybrid_assemble(pairs, pidx, r0, r1, num_corr, true_ratio, rng, rng_stream, idx0, idx1):
    _call('jamie_hybrid_assemble', ptr(pairs), ptr(pidx), ptr(r0), ptr(r1), idx0.numel(), int(num_corr), float(true_ratio),
          ptr(rng), int(rng_stream), ptr(idx0), ptr(idx1), _stream())

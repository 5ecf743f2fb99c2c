"""`JAMIE` facade with the reference's constructor and method surface (reference jamie/jamie.py:29-972)
for the coupled-VAE path: `fit_transform` / `fit`, `transform`, `transform_one`, `modal_predict` /
`impute`, `save_model`, `load_model`, `loss_history`.

Scope: `project_mode='jamie'`.  The correspondence `F` is absent (`use_f_tilde=False`), supplied as `match_result`, or
computed like the reference does: stage A (`compute_distances`, jamie.py:839-890) on the host and stage B
(`match` / `Prime_Dual`, jamie.py:224-414) on the GPU (jamie_amd/correspondence.py).
Unlike the reference no N x N matrix is ever formed when `P` is the identity (the reference's default for
equally sized datasets, jamie.py:425-426): the B x B block `P[idx][:, idx]` is index equality.
"""
import random
import warnings

import numpy as np
import scipy.sparse as sp
import torch

from . import _native as nv
from . import distributed as jd
from .engine import LOSS_NAMES, TrainEngine, kl_anneal
from .model import edModelVar
from .utilities import preclass, time_logger

_DISTANCE_MODES = [
    'euclidean', 'l2', 'l1', 'manhattan', 'cityblock', 'braycurtis', 'canberra', 'chebyshev', 'correlation',
    'cosine', 'dice', 'hamming', 'jaccard', 'kulsinski', 'mahalanobis', 'matching', 'minkowski',
    'rogerstanimoto', 'russellrao', 'seuclidean', 'sokalmichener', 'sokalsneath', 'sqeuclidean', 'yule',
    'wminkowski', 'nan_euclidean', 'haversine', 'geodesic', 'spearman', 'pearson']
# the modes of distances='device' (jamie_amd/distances.py)
_DEVICE_DISTANCE_MODES = ('geodesic', 'euclidean', 'l2', 'sqeuclidean', 'cosine', 'correlation', 'pearson', 'manhattan', 'l1',
                          'cityblock', 'chebyshev')


def _dense_host(x):
    """A modality as a host array: a scipy sparse matrix is densified."""
    return x.toarray() if sp.issparse(x) else np.asarray(x)


def init_random_seed(manual_seed):
    """unioncom.utils.init_random_seed (called at reference jamie.py:142): seeds python `random` and torch."""
    seed = random.randint(1, 10000) if manual_seed is None else manual_seed
    print('use random seed: {}'.format(seed))
    random.seed(seed)
    torch.manual_seed(seed)
    return seed


class JAMIE:
    """MI355X drop-in for `jamie.JAMIE` (coupled-VAE path).

    Constructor keywords are the reference's (jamie.py:38-63) plus the UnionCom keywords it forwards
    (jamie.py:99-111; defaults from unioncom==0.4.0).  Extra, MI355X-only keywords:
      sampler      'auto' (default): 'device' -- Philox batch sampler on the GPU, the step replayed from a recorded launch
                   plan, no host work per step -- unless an explicit-noise seam is installed (`_noise_source`, the fixture
                   replays), then 'numpy'; 'numpy': the reference's `np.random.choice` index stream under `np.random.seed`
                   (drawn on the host every step: ~1 ms at 100k cells); 'device'.  Dropout masks and the reparameterisation noise
                   come from device Philox streams either way, so a production run does not replay the reference's numbers
                   whichever sampler draws the rows: the numpy stream matters to the fixture replays only
      distributed  True -> one process per GPU under torchrun; cells are sharded by rows and the flat
                   gradient is all-reduced once per step over RCCL
      compute_dtype 'f32' (default: exact-fp32 MFMA, the parity configuration) or 'bf16' (bf16 MFMA GEMMs with
                   fp32 accumulation, master weights, optimiser, BatchNorm and losses; feature counts, latent
                   size and batch size must be multiples of 8)
      dp_optimizer 'replicated' (default), 'sharded' or 'auto' (distributed runs): replicated = ONE all-reduce of the flat
                   gradient per step and the full update on every rank (the arrangement north_star names; the only one that
                   has run on more than one GPU over RCCL so far); sharded = the large gradient regions are
                   reduce-scattered, every rank runs clip + Adam over 1/world of the large weight matrices and the updated
                   weights are all-gathered under the next forward pass (distributed.ShardedGradExchange); auto = sharded
                   where it applies (batch_step=True, a world size that divides the regions, no transposed weight copies),
                   else replicated.  With the sharded optimiser `save_checkpoint` / evaluation gather the packed state with
                   collectives: every rank must call them
      grad_comm_dtype 'auto' (default: the compute dtype), 'f32' or 'bf16': precision of the gradient all-reduce
                   messages when distributed (bf16 halves the 4 P bytes exchanged per step)
      distances    'host' (default): stage A (`compute_distances`) on the host in float64 with scipy / sklearn, as the reference;
                   'device': on the MI355X (jamie_amd/distances.py) in fp32 for distance_mode 'geodesic', 'euclidean', 'l2',
                   'sqeuclidean', 'cosine', 'correlation', 'pearson', 'manhattan' / 'l1' / 'cityblock' and 'chebyshev' (any other
                   mode, 'spearman' included, raises ValueError; so does a constant row under 'correlation' / 'pearson', where
                   the host path returns NaN): `self.dist` then holds float32 device tensors that go straight into Prime_Dual,
                   so no N x N matrix crosses PCIe
      metrics      'host' (default): `test_closer` / `test_LabelTA` on the host with sklearn in float64, as the reference (a
                   2N x 2N distance matrix: a few thousand cells at most); 'device': on the MI355X (jamie_amd/metrics.py)
                   in fp32 without any N x N matrix, euclidean only, for whole data sets.  `test_imputation` (per-feature
                   correlation, MSE and AUROC of imputed against measured values): 'host' float64 numpy and sklearn
                   `roc_auc_score`, 'device' jamie_amd/imputation.py (fp64 sums, exact integer rank counts).  `rank_features`
                   (marker features of every group against the rest: Wilcoxon rank sums, Welch's t): 'host' float64 numpy with
                   `scipy.stats.rankdata`, 'device' jamie_amd/markers.py (exact integer rank sums, fp64 moments).  `test_silhouette`
                   (silhouette widths of the pooled cells by label, and by modality within every label; needs no paired cells):
                   'host' sklearn `silhouette_samples` on the N x N distances in float64, 'device' jamie_amd/metrics.py
                   `silhouette` (fp32 distances summed per cell and class in fp64, no N x N matrix).  `test_lisi` (iLISI over the
                   modality and cLISI over the label, Korsunsky et al. 2019) and `neighbors` (the kNN graph of the pooled cells
                   as scipy CSR): 'host' float64 numpy on the N x N distances with a stable argsort, 'device'
                   jamie_amd/neighbors.py (a self search in fp32 that excludes the cell by index, up to 128 neighbours, and
                   the perplexity solve in fp64, no N x N matrix)
      preprocess   'host' (default): `preclass` / sklearn PCA in float64 numpy on the host, the reference's arithmetic; 'device':
                   per-feature statistics and standardisation (or randomized PCA where `pca_dim` names a dimension) on the GPU,
                   written straight into the resident training matrices

    Sparse input.  Every modality handed to `fit` / `fit_transform` / `transform` / `transform_one` / `modal_predict` (`impute`) may
    be a scipy sparse matrix [cells, features] (any format; also behind an AnnData-like object's `.X`), of float or integer values.
    With preprocess='device', fitting uploads the CSR arrays as they are, with no dense copy of the INPUT on the host or the device.
    Without a `pca_dim` for that modality the statistics are taken from the stored entries and the standardised fp32 training matrix
    is written on the GPU (jamie_amd/sparse_input.py); with a `pca_dim` (the default) the randomized PCA runs on the CSR / CSC arrays
    with implicit centring (jamie_amd/pca.py, jamie_amd/sparse_pca.py) and only the [cells, pca_dim] scores are dense.  Either way
    the fp32 training cells come back as `self.dataset`, as for dense input: the reference keeps the transformed cells.  With
    preprocess='host' fitting DENSIFIES ON THE HOST (`X.toarray()`) and follows the dense path.  `transform` / `transform_one` /
    `modal_predict` stream row chunks of the CSR matrix through the GPU whatever `preprocess` was -- through the PCA's components
    for a modality fitted on the device -- unless the modality carries an sklearn PCA (preprocess='host' with a `pca_dim`: then
    `toarray()`); the result equals the dense call's within the inference tolerance.
    """

    def __init__(self, match_result=None, PF_Ratio=None, corr_method='unioncom', dist_method='euclidean',
                 in_place=False, loss_weights=None, model_pca='pca', model_class=edModelVar, model_lr=1e-3,
                 dropout=None, pca_dim=2 * [512], batch_step=True, use_f_tilde=True, use_early_stop=True,
                 min_epochs=2500, min_increment=1e-8, max_steps_without_increment=500, debug=False,
                 log_debug=100, record_loss=True, enable_memory_logging=False, device='cuda',
                 sampler='auto', distributed=False, compute_dtype='f32', grad_comm_dtype='auto', dp_optimizer='replicated',
                 preprocess='host', checkpoint_path=None, checkpoint_every=0, distances='host', metrics='host',
                 **kwargs):
        self.match_result = match_result
        self.PF_Ratio = PF_Ratio
        self.corr_method = corr_method
        self.dist_method = dist_method
        self.in_place = in_place
        self.loss_weights = loss_weights
        self.model_pca = model_pca
        self.model_class = model_class
        self.model_lr = model_lr
        self.dropout = dropout
        self.pca_dim = pca_dim
        self.batch_step = batch_step
        self.use_f_tilde = use_f_tilde
        self.use_early_stop = use_early_stop
        self.min_epochs = min_epochs
        self.min_increment = min_increment
        self.max_steps_without_increment = max_steps_without_increment
        self.debug = debug
        self.log_debug = log_debug
        self.record_loss = record_loss
        self.enable_memory_logging = enable_memory_logging
        if device == 'cpu':
            raise nv.JamieHipError("jamie_amd runs on the MI355X only; use device='cuda' (no CPU fallback)")
        self.device = device
        if sampler not in ('auto', 'numpy', 'device'):
            raise ValueError("sampler must be 'auto', 'numpy' or 'device'")
        self.sampler = sampler
        self.distributed = distributed
        self.compute_dtype = compute_dtype
        if preprocess not in ('host', 'device'):
            raise ValueError("preprocess must be 'host' (numpy fp64, the reference's arithmetic) or 'device'")
        self.preprocess = preprocess
        if distances not in ('host', 'device'):
            raise ValueError("distances must be 'host' (scipy / sklearn in float64, the reference's arithmetic) or 'device'")
        self.distances = distances
        if metrics not in ('host', 'device'):
            raise ValueError("metrics must be 'host' (sklearn in float64, the reference's arithmetic) or 'device'")
        self.metrics = metrics
        # training checkpoints (the reference only pickles the finished model, jamie.py:967-972):
        # every `checkpoint_every` epochs the full training state goes to `checkpoint_path`;
        # fit_transform(..., resume_from=path) continues from it and ends bit-identical to an uninterrupted run
        self.checkpoint_path, self.checkpoint_every = checkpoint_path, int(checkpoint_every or 0)
        self._resume_from = None
        if grad_comm_dtype not in ('auto', 'f32', 'bf16'):
            raise ValueError("grad_comm_dtype must be 'auto', 'f32' or 'bf16'")
        if dp_optimizer not in ('auto', 'sharded', 'replicated'):
            raise ValueError("dp_optimizer must be 'auto', 'sharded' or 'replicated'")
        self.dp_optimizer = dp_optimizer
        self.grad_comm_dtype = compute_dtype if grad_comm_dtype == 'auto' else grad_comm_dtype
        # UnionCom attributes (reference jamie.py:99-111 defaults, then unioncom 0.4.0's)
        defaults = {'project_mode': 'jamie', 'log_pd': 500, 'lr': 1e-3, 'epoch_DNN': 10000, 'log_DNN': 500,
                    'batch_size': 512, 'epoch_pd': 2000, 'epsilon': 1e-3, 'rho': 10, 'beta': 1, 'perplexity': 30,
                    'manual_seed': 666, 'delay': 0, 'kmax': 40, 'output_dim': 32, 'distance_mode': 'geodesic',
                    'integration_type': 'MultiOmics'}
        for k, v in defaults.items():
            setattr(self, k, kwargs.pop(k, v))
        if kwargs:
            raise TypeError(f'unexpected keyword arguments: {sorted(kwargs)}')
        if self.distances == 'device' and self.distance_mode not in _DEVICE_DISTANCE_MODES:
            raise ValueError(f"distances='device' supports distance_mode {', '.join(map(repr, _DEVICE_DISTANCE_MODES))}; "
                             f"got {self.distance_mode!r} (use distances='host')")
        self.model = None
        self.engine = None
        self.loss_history = {}
        # test seam: callable(step_number) -> {'eps', 'enc_masks', 'dec_masks'} device tensors fed to the step instead of
        # the Philox streams, so that the loop users call can be replayed against the reference's fixtures
        self._noise_source = None

    # ------------------------------------------------------------------------------------------
    def fit_transform(self, dataset=None, P=None, resume_from=None):
        """reference jamie.py:113-222.  `resume_from`: a checkpoint written by this class (`checkpoint_path`)."""
        self.P = P
        self._resume_from = resume_from
        if self.integration_type not in ['MultiOmics']:
            raise Exception('integration_type error! Enter MultiOmics.')
        if self.distance_mode not in _DISTANCE_MODES:
            raise Exception('distance_mode error! Enter a correct distance_mode.')
        if self.project_mode not in ('jamie', 'tsne'):
            raise Exception("Choose correct project_mode: 'nlma', 'tsne'.")
        assert self.model_pca in ('pca', 'umap')
        if self.project_mode == 'tsne':
            raise NotImplementedError("project_mode='tsne' is outside the accelerated path (SURVEY.md §8)")
        time = time_logger(memory_usage=self.enable_memory_logging, sync=torch.cuda.synchronize)   # jamie.py:141
        init_random_seed(self.manual_seed)                         # jamie.py:142
        self.dataset = dataset
        self.dataset_annotation = None
        if hasattr(self.dataset[0], 'X') and not isinstance(self.dataset[0], np.ndarray):   # AnnData
            self.dataset = [d.X for d in self.dataset]
            self.dataset_annotation = dataset
        if not self.in_place:
            self.dataset = self.dataset * 1                        # shallow copy, jamie.py:152-153
        self.dataset_num = len(self.dataset)
        self.row = [np.shape(d)[0] for d in self.dataset]
        self.col = [np.shape(d)[1] for d in self.dataset]
        # stage A (host, as in the reference) and stage B (Prime_Dual on the GPU): jamie.py:162-177
        if self.match_result is None and self.use_f_tilde:
            if self.dataset_num != 2:
                raise NotImplementedError('use_f_tilde=True follows the reference: two modalities')
            self.compute_distances(save_dist=True)
        time.log('Distance')
        if self.match_result is None and self.use_f_tilde:
            self.match_result = self.match()
        time.log('Correspondence')
        integrated = self.project_jamie()
        time.log('Mapping')
        print('-' * 33)
        print('JAMIE Done!')
        time.aggregate()
        print()
        return integrated

    # ---- stages A / B (reference jamie.py:224-249, 314-414, 839-890) ----
    def compute_distances(self, save_dist=True):
        """Cell x cell distance matrix of every modality (host numpy / scipy / sklearn, as in the reference; with
        distances='device' float32 device tensors from jamie_amd/distances.py)."""
        from .utilities import distance_matrix
        if save_dist:
            self.dist = []
        print('Shape of Raw data')
        for i in range(self.dataset_num):
            print('Dataset {}:'.format(i), np.shape(self.dataset[i]))
        if self.distances == 'device':
            self.distance_function = self._device_distance_function()
        else:
            self.distance_function = lambda df: distance_matrix(df, self.distance_mode, self.kmax)   # noqa: E731
        if save_dist:
            self.dist = [self.distance_function(d) for d in self.dataset]

    def _device_distance_function(self):
        from . import distances as jdist
        mode = self.distance_mode
        if mode not in _DEVICE_DISTANCE_MODES:
            raise ValueError(f"distances='device' supports distance_mode {', '.join(map(repr, _DEVICE_DISTANCE_MODES))}; "
                             f"got {mode!r} (use distances='host')")
        if mode == 'geodesic':
            return lambda df: jdist.geodesic(df, self.kmax, device=self.device)            # noqa: E731
        other = {'cosine': jdist.cosine, 'correlation': jdist.correlation, 'pearson': jdist.pearson, 'manhattan': jdist.manhattan,
                 'l1': jdist.manhattan, 'cityblock': jdist.manhattan, 'chebyshev': jdist.chebyshev}.get(mode)
        if other is not None:
            return lambda df: other(df, device=self.device)                                # noqa: E731
        return lambda df: jdist.euclidean(df, squared=mode == 'sqeuclidean', device=self.device)   # noqa: E731

    def Prime_Dual(self, dist, dx=None, dy=None, verbose=True):
        """reference jamie.py:314-414, on the MI355X (jamie_amd/correspondence.py); returns F as numpy float32."""
        from .correspondence import prime_dual
        if self.integration_type != 'MultiOmics':
            raise NotImplementedError("Prime_Dual: integration_type 'MultiOmics' (the only one fit_transform accepts)")
        return prime_dual(dist, dx, dy, epoch_pd=self.epoch_pd, rho=self.rho, epsilon=self.epsilon, delay=self.delay,
                          log_pd=self.log_pd, verbose=verbose, device=self.device)

    def match(self):
        """reference jamie.py:224-249."""
        print('Device:', self.device)
        cor_pairs = []
        for i in range(self.dataset_num):
            for j in range(i + 1, self.dataset_num):
                print('-' * 33)
                print(f'Find correspondence between Dataset {i + 1} and Dataset {j + 1}')
                if self.corr_method != 'unioncom':
                    raise NotImplementedError("corr_method='jamie' is a work in progress in the reference "
                                              '(jamie.py:241-246) and is not built')
                cor_pairs.append(self.Prime_Dual([self.dist[i], self.dist[j]], dx=self.col[i], dy=self.col[j]))
        print('Finished Matching!')
        return cor_pairs

    def fit(self, dataset=None, P=None, resume_from=None):
        """north_star spelling: train, return self."""
        self._last_embedding = self.fit_transform(dataset, P, resume_from=resume_from)
        return self

    # ------------------------------------------------------------------------------------------
    def _build_preprocessing(self):
        """reference jamie.py:434-469.  A scipy sparse modality is densified on the host first."""
        pre = []
        if self.pca_dim is not None:
            for dim, data in zip(self.pca_dim, self.dataset):
                data = _dense_host(data)
                if dim is not None:
                    from sklearn.decomposition import PCA
                    if min(*data.shape) < dim:
                        warnings.warn(f'PCA dim must be lower than {min(*data.shape)}, found {dim}, '
                                      f'adjusting to compensate.')
                        dim = min(*data.shape)
                    if self.model_pca != 'pca':
                        raise NotImplementedError("model_pca='umap' needs umap-learn (absent)")
                    pca = PCA(n_components=dim)
                    sample = pca.fit_transform(data)
                    pre.append(preclass(sample, pca=pca))
                else:
                    pre.append(preclass(np.asarray(data), axis=0))
        else:
            pre = [preclass(_dense_host(d), axis=0) for d in self.dataset]
        return pre

    def project_jamie(self, W=None):
        """The training loop, reference jamie.py:416-804."""
        print('-' * 33)
        print('Train coupled autoencoders')
        # the reference asserts two modalities (jamie.py:420); 3-4 fully paired ones run the build-defined
        # generalisation (identity correspondence, F = 0)
        assert 2 <= self.dataset_num <= 4, 'Currently only compatible with 2 (reference) to 4 modalities.'
        if self.dataset_num > 2 and (self.P is not None or self.use_f_tilde or len(set(self.row)) != 1):
            raise NotImplementedError('more than two modalities need fully paired cells (P=None, use_f_tilde=False)')
        dev = torch.device(self.device)
        rank, world = 0, 1
        allreduce = None
        if self.distributed:
            rank, world, _ = jd.init_from_env()
            allreduce = jd.OverlappedGradAllReduce(comm_dtype=torch.bfloat16 if self.grad_comm_dtype == 'bf16' else None)
        # ---- P / F (never densified for the identity) ----
        P_dense = P_csr = None
        if self.P is None:
            method = 'diag' if self.row[0] == self.row[1] else 'zeros'      # jamie.py:423-428, 518-533
        elif sp.issparse(self.P):
            # sparse partial correspondence: CSR on the device, the B x B block of a batch is
            # looked up by jamie_csr_block -- no N x N array at any point
            Pc = sp.csr_matrix(self.P, dtype=np.float32)
            Pc.sum_duplicates()
            Pc.sort_indices()
            if Pc.shape[0] == Pc.shape[1] and Pc.nnz == Pc.shape[0] and bool((Pc.diagonal() == 1).all()):
                method = 'diag'
            elif Pc.nnz and float(np.abs(Pc.data).sum()) != 0:
                method = 'hybrid'                                             # corrected sampler, see the dense branch
                coo = Pc.tocoo()
                keep = coo.data > 0
                self.corr_samples = np.stack([coo.row[keep], coo.col[keep]], axis=1)
                self.num_corr = len(self.corr_samples)
                self.true_ratio = .8                                          # jamie.py:529
                P_csr = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in
                              (Pc.indptr.astype(np.int32), Pc.indices.astype(np.int32), Pc.data.astype(np.float32)))
            else:
                method = 'zeros'
        else:
            P_dense = torch.as_tensor(np.asarray(self.P), dtype=torch.float32, device=dev)
            if P_dense.shape[0] == P_dense.shape[1] and torch.abs(
                    P_dense - torch.eye(self.row[0], device=dev)).sum() == 0:
                method, P_dense = 'diag', None
            elif torch.abs(P_dense).sum() != 0:
                # partial correspondence (reference jamie.py:523-530), CORRECTED: the reference sets
                # `num_corr = len(corr_samples[0])` (== 2, the pair width) and indexes `corr_samples[i]` (the i-th
                # pair) per modality, so it never samples the known pairs as intended; here num_corr is the number
                # of known pairs and column i of the pair list feeds modality i.
                method = 'hybrid'
                self.corr_samples = np.argwhere(np.asarray(self.P) > 0)
                self.num_corr = len(self.corr_samples)
                self.true_ratio = .8                                          # jamie.py:529
            else:
                method = 'zeros'
        self.sampling_method = method
        F_dense = None
        if self.use_f_tilde:
            mr = self.match_result[0]
            F_dense = (mr.to(dev, torch.float32) if torch.is_tensor(mr)
                       else torch.as_tensor(np.asarray(mr), dtype=torch.float32, device=dev))
        timer = time_logger(memory_usage=self.enable_memory_logging, sync=torch.cuda.synchronize)    # jamie.py:433
        # per-step labels of the reference ('Get subset samples', 'Step'; jamie.py:601, 742): a synchronising timer inside
        # the loop would block the host twice per step, so it only runs when `debug` asks for the per-phase table
        step_timer = timer if self.debug else time_logger(record=False)
        # ---- preprocessing (host, numpy/sklearn like the reference) ----
        dev_pre = self.preprocess == 'device'
        if dev_pre:
            # on the GPU: per-feature standardisation (jamie_col_stats / jamie_standardise: fp64
            # statistics in numpy's two-pass order) or, where `pca_dim` names a dimension (the reference's default,
            # jamie.py:50, 436-457), randomized PCA on the fp32 MFMA GEMM (jamie_amd/pca.py) followed by the global
            # scaling of `preclass(sample, pca=pca)`; fp32 cells are written straight into the resident training matrices.
            # The host keeps the `preclass` objects (statistics, fitted PCA) for transform / inverse_transform of new data
            from .pca import DevicePCA, global_standardise
            pre, data_dev = [], []
            dims_pca = self.pca_dim if self.pca_dim is not None else [None] * len(self.dataset)
            for dim, x in zip(dims_pca, self.dataset):
                if sp.issparse(x):
                    if dim is None:
                        # CSR arrays to the GPU as they are: statistics from the stored entries, dense fp32 rows written there
                        from .sparse_input import standardise_csr
                        out, mean, sd = standardise_csr(x, dev)
                        pre.append(preclass.from_stats(mean.cpu().numpy(), sd.cpu().numpy(), axis=0))
                        data_dev.append(out)
                        continue
                    # ... and through the PCA too: its products run on the CSR / CSC arrays (jamie_amd/sparse_pca.py)
                    if self.model_pca != 'pca':
                        raise NotImplementedError("model_pca='umap' needs umap-learn (absent)")
                    if min(*x.shape) < dim:
                        warnings.warn(f'PCA dim must be lower than {min(*x.shape)}, found {dim}, '
                                      f'adjusting to compensate.')
                        dim = min(*x.shape)
                    pca = DevicePCA(dim, device=self.device)
                    out, m, sdev = global_standardise(pca.fit_transform_device(x))
                    pre.append(preclass.from_stats(m, sdev, axis=None, pca=pca))
                    data_dev.append(out)
                    continue
                xa = np.ascontiguousarray(np.asarray(x))
                if xa.dtype not in (np.float32, np.float64):
                    xa = xa.astype(np.float64)
                if dim is None:
                    out, mean, sd = nv.standardise_columns(torch.from_numpy(xa).to(dev))
                    pre.append(preclass.from_stats(mean.cpu().numpy(), sd.cpu().numpy(), axis=0))
                else:
                    if self.model_pca != 'pca':
                        raise NotImplementedError("model_pca='umap' needs umap-learn (absent)")
                    if min(*xa.shape) < dim:
                        warnings.warn(f'PCA dim must be lower than {min(*xa.shape)}, found {dim}, '
                                      f'adjusting to compensate.')
                        dim = min(*xa.shape)
                    pca = DevicePCA(dim, device=self.device)        # random_state=None: numpy's global RNG, like sklearn's
                    out, m, sdev = global_standardise(pca.fit_transform_device(torch.from_numpy(xa).to(dev)))
                    pre.append(preclass.from_stats(m, sdev, axis=None, pca=pca))
                data_dev.append(out)
            self.dataset = [d.cpu().numpy() for d in data_dev]                # the reference keeps the transformed cells
        else:
            self.dataset = [_dense_host(x) for x in self.dataset]            # (sparse input: densified on the host, once)
            pre = self._build_preprocessing()
            self.dataset = [p.transform(np.asarray(x)) for p, x in zip(pre, self.dataset)]
        self.col = [x.shape[1] for x in self.dataset]
        # ---- model / engine ----
        extra = {}
        if self.compute_dtype == 'bf16' and self.model_class is edModelVar and any(c % 8 for c in self.col):
            extra['pad_features'] = 8        # bf16 GEMM operands need feature counts that are multiples of 8 (model.py)
        self.model = self.model_class(self.col, self.output_dim, preprocessing=[p.transform for p in pre],
                                      preprocessing_inverse=[p.inverse_transform for p in pre],
                                      dropout=self.dropout, **extra).to(self.device)
        if world > 1:
            jd.broadcast_flat(self.model.flat)
        self.model.train()
        data_all = data_dev if dev_pre else [torch.from_numpy(np.ascontiguousarray(x)).float() for x in self.dataset]
        # row shards for data parallelism ('diag' keeps the same rows of both modalities on one rank)
        bounds = [jd.shard_bounds(r, rank, world) for r in self.row]
        data = [d[lo:hi].to(dev).contiguous() for d, (lo, hi) in zip(data_all, bounds)]
        rows = [hi - lo for lo, hi in bounds]
        # every rank must run the same number of steps per epoch (each step is a collective) with the same batch size:
        # both follow from the SMALLEST shard (shard sizes differ by at most one row), not from this rank's own
        rows_all = [[b[1] - b[0] for b in (jd.shard_bounds(r, k, world) for r in self.row)] for k in range(world)]
        len_dataloader = min(int(np.max(rk) / self.batch_size) for rk in rows_all)   # jamie.py:511-514
        if len_dataloader == 0:
            len_dataloader = 1
            self.batch_size = min(int(np.max(rk)) for rk in rows_all)
        B = int(self.batch_size)
        if method == 'hybrid' and world > 1:
            # data parallel partial correspondence: a rank samples the known pairs whose two cells both live in its row
            # shards (contiguous shards of every modality; a pair that straddles two ranks is only reachable through the
            # unpaired draws of its two cells); indices become shard-local
            cs = self.corr_samples
            keep = ((cs[:, 0] >= bounds[0][0]) & (cs[:, 0] < bounds[0][1]) & (cs[:, 1] >= bounds[1][0]) & (cs[:, 1] < bounds[1][1]))
            self.corr_samples = cs[keep] - np.array([bounds[0][0], bounds[1][0]])
            self.num_corr = len(self.corr_samples)
            if self.num_corr == 0:
                raise ValueError(f'rank {rank}: no known pair lies inside its row shards; shard paired cells together')
        self.PF_Ratio = 1 if self.PF_Ratio is None else self.PF_Ratio        # jamie.py:517
        eng = TrainEngine(self.model, B, lr=self.model_lr, loss_weights=self.loss_weights,
                          dist_method=self.dist_method, seed=int(self.manual_seed) + 7919 * rank,
                          world_size=world, compute_dtype=self.compute_dtype, torch_one_minus_beta=True)
        eng.accumulate = False
        if not self.batch_step:
            eng.set_grad_bf16(False)        # gradients accumulate over the batches of an epoch (jamie.py:734-749): fp32 buffer
        self.engine = eng
        data = eng.pad_cells(data)
        rep = min(self.col) < B and self.dataset_num == 2                    # jamie.py:553 (sic); M > 2: never
        need_block = ((method == 'diag' and rep) or method == 'zeros' or F_dense is not None or P_dense is not None
                      or P_csr is not None or self.PF_Ratio != 1)
        if self.dataset_num > 2 and need_block:
            raise NotImplementedError('more than two modalities: min(features) must be >= batch_size (no duplicates)')
        idx_dev = [torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(self.dataset_num)]
        blk_F = torch.empty(B, B, device=dev) if F_dense is not None else None
        blk_mix = torch.empty(B, B, device=dev) if self.PF_Ratio != 1 else None
        best_running_loss = np.inf
        streak = 0
        if self.record_loss:
            self.loss_history = {}
        # fast path: device sampler, 'diag' sampling, no dense P/F blocks -> the step is a fixed launch sequence on
        # static buffers: record it once and replay it (one foreign call per launch, nothing rebuilt per step)
        plan = None
        sampler = self.sampler if self.sampler != 'auto' else ('numpy' if self._noise_source is not None else 'device')
        use_plan = (sampler == 'device' and method == 'diag' and P_dense is None and F_dense is None
                    and P_csr is None and self.PF_Ratio == 1 and self.batch_step)
        # partial correspondence from a sparse P with the device sampler: pair / rest candidates from jamie_sample_indices,
        # jamie_hybrid_assemble picks per slot, jamie_csr_block builds the [B,B] block -- the whole step stays on the GPU and
        # is recorded as a plan too (the numpy sampler costs 2 ms of host time per step at 100k cells: np.random.choice without
        # replacement permutes all N rows)
        plan_hybrid = (sampler == 'device' and method == 'hybrid' and P_csr is not None and F_dense is None
                       and self.PF_Ratio == 1 and self.batch_step and world == 1 and B <= 2048)
        if plan_hybrid:
            pairs_dev = torch.from_numpy(np.ascontiguousarray(self.corr_samples.astype(np.int32))).to(dev)
            hy = [torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(3)]

            def hybrid_step():
                nv.sample_indices_group([nv.sample_args(hy[0], self.num_corr, 0, rep or self.num_corr < B, 202),
                                         nv.sample_args(hy[1], rows[0], 0, rep, 200),
                                         nv.sample_args(hy[2], rows[1], 0, rep, 201)], eng.state)
                nv.hybrid_assemble(pairs_dev, hy[0], hy[1], hy[2], self.num_corr, self.true_ratio, eng.state, 203,
                                   idx_dev[0], idx_dev[1])
                eng.load_batch(data, idx_dev)
                nv.csr_block(*P_csr, idx_dev[0], idx_dev[1], eng.corr, bounds[0][0], bounds[1][0])
                eng.step(eng.corr, None, None, allreduce)
        epoch_sum = torch.zeros((), device=dev)      # batch_step=False: epoch loss = mean of the batch losses (jamie.py:728)
        start_epoch = 0
        if self._resume_from is not None:
            start_epoch, best_running_loss, streak = self._load_checkpoint(self._resume_from, eng)
            self._resume_from = None
        if allreduce is not None and world > 1 and self.dp_optimizer != 'replicated' and self.batch_step:
            # (after a resume: the packed pieces are cut from the restored parameters and moments)
            try:
                ex = jd.ShardedGradExchange(comm_dtype=allreduce.comm_dtype)
                eng.enable_sharded_optimizer(ex)
                allreduce = ex
            except ValueError:
                if self.dp_optimizer == 'sharded':
                    raise
        timer.log('Setup')
        n_steps = start_epoch * len_dataloader
        if self._noise_source is not None and (use_plan or plan_hybrid):
            raise ValueError('explicit noise needs the eager path (sampler="numpy")')
        for epoch in range(start_epoch, self.epoch_DNN):                      # jamie.py:546
            eng.set_kl_anneal(kl_anneal(epoch, self.min_epochs, self.epoch_DNN))
            eng.reset_best()
            for batch_idx in range(len_dataloader):
                if use_plan:
                    if plan is None:
                        plan = eng.make_plan(data, idx_dev[0], rows[0], rep, allreduce)
                    else:
                        eng.run_plan(plan)
                    continue
                if plan_hybrid:
                    if plan is None:
                        nv.begin_record()
                        try:
                            hybrid_step()                  # the recording step is a real step
                        finally:
                            plan = nv.end_record()
                    else:
                        eng.run_plan(plan)
                    continue
                # ---- sampler (jamie.py:552-583) ----
                if method == 'hybrid':                                         # jamie.py:559-573 (corrected)
                    corr_sample_num = int(min(np.sum(np.random.rand(B) < self.true_ratio), self.num_corr))
                    pairs = self.corr_samples[np.random.choice(self.num_corr, corr_sample_num, replace=rep)]
                    for i in range(2):
                        rest = np.random.choice(rows[i], B - corr_sample_num, replace=rep)
                        s = np.concatenate([pairs[:, i], rest], axis=0)
                        idx_dev[i].copy_(torch.from_numpy(s.astype(np.int32)))
                elif sampler == 'numpy':
                    if method == 'diag':
                        s = np.random.choice(rows[0], B, replace=rep)      # (= choice(range(N), ...): the same stream
                                                                           #  without the 100k-element list conversion)
                        idx_dev[0].copy_(torch.from_numpy(s.astype(np.int32)))
                        for j in range(1, self.dataset_num):
                            idx_dev[j].copy_(idx_dev[0])
                    else:
                        for i in range(2):
                            s = np.random.choice(rows[i], B, replace=rep)
                            idx_dev[i].copy_(torch.from_numpy(s.astype(np.int32)))
                else:
                    nv.sample_indices(idx_dev[0], rows[0], 0, rep, eng.state, 200)
                    if method == 'diag':
                        for j in range(1, self.dataset_num):
                            idx_dev[j].copy_(idx_dev[0])
                    else:
                        nv.sample_indices(idx_dev[1], rows[1], 0, rep, eng.state, 201)
                eng.load_batch(data, idx_dev)
                # ---- P / F blocks (jamie.py:585-604) ----
                corr = Fblk = None
                if need_block:
                    if P_csr is not None:
                        nv.csr_block(*P_csr, idx_dev[0], idx_dev[1], eng.corr, bounds[0][0], bounds[1][0])
                    elif P_dense is not None:         # one B x B gather + row normalisation (no [B, N] slab)
                        nv.dense_block(P_dense, idx_dev[0], idx_dev[1], eng.corr, bounds[0][0], bounds[1][0])
                    elif method == 'diag':
                        nv.corr_from_indices(idx_dev[0], idx_dev[1], eng.corr)
                    else:
                        eng.corr.zero_()
                    corr = eng.corr
                    if F_dense is not None:
                        nv.dense_block(F_dense, idx_dev[0], idx_dev[1], blk_F, bounds[0][0], bounds[1][0])
                        Fblk = blk_F
                    if self.PF_Ratio != 1:                                     # jamie.py:604
                        nv.axpby(blk_mix, self.PF_Ratio, eng.corr, 1 - self.PF_Ratio, Fblk)
                        corr = blk_mix
                step_timer.log('Get subset samples')
                noise = None if self._noise_source is None else self._noise_source(n_steps)
                n_steps += 1
                if self.batch_step:
                    eng.step(corr, Fblk, noise, allreduce)
                else:
                    # jamie.py:734-749: every batch back-propagates into the same gradient buffers, ONE clip + Adam
                    # step per epoch; the gradient all-reduce rides on the last batch's backward
                    last = batch_idx == len_dataloader - 1
                    eng.accumulate = batch_idx > 0
                    eng.forward_backward(corr, Fblk, noise, allreduce if last else None)
                    epoch_sum += eng.losses[4]
                    if not last:
                        eng.state[0] += 1          # the Philox step only advances with the optimiser: fresh noise per batch
                    else:
                        eng.state[0] -= len_dataloader - 1
                    if last:
                        if allreduce is not None:
                            allreduce.finish() if hasattr(allreduce, 'finish') else allreduce(eng.grad)
                        eng.accumulate = False
                        eng.optimizer_step()
                step_timer.log('Step')
            # ---- per-epoch bookkeeping (one device read per epoch; jamie.py:751-792) ----
            ls, total, best_batch_loss = eng.read_losses()
            if not self.batch_step:                    # jamie.py:778-781: the early-stop criterion is the epoch loss
                best_batch_loss = total = float(epoch_sum) / len_dataloader
                epoch_sum.zero_()
            if self.record_loss:
                for name, lo in zip(LOSS_NAMES, ls):
                    self.loss_history.setdefault(name, []).append(lo)
            if (epoch + 1) % self.log_debug == 0 and self.debug:
                print('  '.join(f'{n}: {lo:.4f}' for n, lo in zip(LOSS_NAMES, ls)))
            if (epoch + 1) % self.log_DNN == 0:
                print(f'epoch:[{epoch + 1:d}/{self.epoch_DNN}]: loss:{total:4f}')
            if epoch > self.min_epochs:
                if world > 1:
                    # the ranks train on different shards, so their losses differ; the stop decision must not (a rank that
                    # left the loop would leave the others waiting in the gradient all-reduce): mean over ranks, one scalar
                    # per epoch, outside the step
                    best_batch_loss = jd.mean_scalar(best_batch_loss, dev)
                if best_running_loss - best_batch_loss > self.min_increment:
                    best_running_loss = best_batch_loss
                    streak = 0
                else:
                    streak += 1
                if streak >= self.max_steps_without_increment and self.use_early_stop:
                    break
            if self.checkpoint_every and self.checkpoint_path and (epoch + 1) % self.checkpoint_every == 0:
                eng.flush(collective=True)       # (every rank: a sharded optimiser gathers its pieces with collectives)
                if world > 1:
                    jd.average_(self.model.bn_flat)
                if rank == 0:
                    self.save_checkpoint(self.checkpoint_path, epoch + 1, best_running_loss, streak)
        eng.flush(collective=True)
        if world > 1:
            # BatchNorm running statistics are per-rank during training (no SyncBN: one collective per step); the model
            # that is evaluated / saved carries their average, so every rank returns the same embeddings
            jd.average_(self.model.bn_flat)
        self.model.eval()
        out = [self.model.embed(data_all[i], i).cpu().numpy() for i in range(self.dataset_num)]   # jamie.py:794-799
        timer.log('Output')
        print('Finished Mapping!')
        if self.debug:
            timer.aggregate()
        return out

    # ------------------------------------------------------------------------------------------
    def _csr_preclass(self, i):
        """The `preclass` of modality i if its fitted preprocessing is plain per-feature standardisation (the only kind sparse rows
        are streamed through), else None.  It is reachable as the bound method's `__self__`, for loaded models too."""
        pre = getattr(self.model.preprocessing[i], '__self__', None)
        if not all(hasattr(self.model, m) for m in ('_encode_eval', '_mu_eval', '_decode_eval')):
            return None                                            # (a model class of the caller's: `toarray()`)
        if isinstance(pre, preclass) and pre.axis == 0 and pre.pca is None:
            return pre
        return None

    def _csr_chunks(self, data, i, pre, chunk):
        """Standardised fp32 device rows of the sparse cells `data` of modality i, `chunk` rows at a time: the CSR arrays of a
        chunk go up and `jamie_csr_standardise` writes (x - mean) / std, NaN -> 0, against the statistics uploaded once."""
        from . import sparse_input as jsp
        A = jsp.canonical_csr(data)
        d = int(np.size(pre.mean))
        if A.shape[1] != d:
            raise ValueError(f'modality {i} was fitted on {d} features, the sparse input has {A.shape[1]}')
        chunk = int(chunk)
        if chunk < 1:
            raise ValueError(f'chunk must be >= 1 row, got {chunk}')
        dev = torch.device(getattr(self.model, 'device', self.device))
        mean = torch.from_numpy(np.ascontiguousarray(np.asarray(pre.mean, dtype=np.float64).reshape(-1))).to(dev)
        sd = torch.from_numpy(np.ascontiguousarray(np.asarray(pre.std, dtype=np.float64).reshape(-1))).to(dev)
        for s in range(0, A.shape[0], chunk):
            yield jsp.apply_csr(A[s:s + chunk], mean, sd, dev, canonical=True)

    def _csr_pca_preclass(self, i):
        """The `preclass` of modality i if its fitted preprocessing is a device PCA followed by the global scaling
        (`preclass(sample, pca=pca)`, axis None, fitted with preprocess='device'), else None: an sklearn PCA takes dense input."""
        from .pca import DevicePCA
        pre = getattr(self.model.preprocessing[i], '__self__', None)
        if not all(hasattr(self.model, m) for m in ('_encode_eval', '_mu_eval', '_decode_eval')):
            return None
        if isinstance(pre, preclass) and pre.axis is None and isinstance(pre.pca, DevicePCA):
            return pre
        return None

    def _csr_pca_chunks(self, data, i, pre, chunk):
        """Scaled PCA scores (fp32 device rows [rows, k]) of the sparse cells `data` of modality i, `chunk` rows at a time: the CSR
        arrays of a chunk go up, `jamie_csr_spmm` takes them against components^T with t = mean^T components^T (uploaded once),
        and `jamie_standardise` writes (score - m) / s, NaN -> 0."""
        from . import sparse_input as jsp
        from .sparse_pca import DeviceCSR, weighted_colsum
        A = jsp.canonical_csr(data)
        pca = pre.pca
        k, d = pca.components_.shape
        if A.shape[1] != d:
            raise ValueError(f'modality {i} was fitted on {d} features, the sparse input has {A.shape[1]}')
        chunk = int(chunk)
        if chunk < 1:
            raise ValueError(f'chunk must be >= 1 row, got {chunk}')
        dev = torch.device(getattr(self.model, 'device', self.device))
        compT = torch.from_numpy(np.ascontiguousarray(pca.components_.T.astype(np.float32))).to(dev)
        t = weighted_colsum(compT, torch.from_numpy(np.ascontiguousarray(pca.mean_, dtype=np.float64)).to(dev))
        m = torch.full((k,), float(pre.mean), dtype=torch.float64, device=dev)
        s = torch.full((k,), float(pre.std), dtype=torch.float64, device=dev)
        for lo in range(0, A.shape[0], chunk):
            part = A[lo:lo + chunk]
            scores = DeviceCSR(part.indptr, part.indices, part.data, d, dev).product(compT, t=t)
            out = torch.empty_like(scores)
            nv._call('jamie_standardise', nv.ptr(scores), 0, scores.shape[0], k, k, nv.ptr(m), nv.ptr(s), nv.ptr(out), nv._stream())
            yield out

    def _sparse_chunks(self, data, i, chunk):
        """The standardised device rows of the sparse cells `data` as the fitted preprocessing of modality i gives them, in row
        chunks, or None where that preprocessing takes dense input only."""
        pre = self._csr_preclass(i)
        if pre is not None:
            return self._csr_chunks(data, i, pre, chunk)
        pre = self._csr_pca_preclass(i)
        if pre is not None:
            return self._csr_pca_chunks(data, i, pre, chunk)
        return None

    def _embed_input(self, data, i, pre_transformed, chunk):
        """`mu` of modality i for dense or sparse cells: a device tensor [cells, output_dim]."""
        if sp.issparse(data):
            chunks = None if pre_transformed else self._sparse_chunks(data, i, chunk)
            if chunks is not None:
                self.model.eval()
                outs = [self.model._mu_eval(i, self.model._encode_eval(i, x)) for x in chunks]
                if outs:
                    return torch.cat(outs, 0) if len(outs) > 1 else outs[0]
            data = data.toarray()                                  # an sklearn PCA, pre-transformed or empty input
        if not pre_transformed:
            data = self.model.preprocessing[i](np.asarray(data))
        self.model.eval()
        # (`chunk` goes to the model only when the caller set it: a `model_class` of the caller's may not take it)
        kw = {} if chunk == 65536 else {'chunk': chunk}
        return self.model.embed(torch.as_tensor(np.asarray(data)).float(), i, **kw)

    def modal_predict(self, data, modality, pre_transformed=False, chunk=65536):
        """reference jamie.py:806-815 (returns float64: the inverse scaling promotes).  `data` may be a scipy sparse matrix; `chunk`:
        rows per pass through the network."""
        assert self.model is not None, 'Model must be trained before modal prediction.'
        to_modality = (modality + 1) % self.dataset_num
        chunks = self._sparse_chunks(data, modality, chunk) if sp.issparse(data) and not pre_transformed else None
        self.model.eval()
        if chunks is not None and data.shape[0] > 0:
            outs = [self.model._decode_eval(to_modality, self.model._mu_eval(modality, self.model._encode_eval(modality, x)))
                    for x in chunks]
            decoded = torch.cat(outs, 0) if len(outs) > 1 else outs[0]
        else:
            if sp.issparse(data):
                data = data.toarray()
            if not pre_transformed:
                data = self.model.preprocessing[modality](np.asarray(data))
            kw = {} if chunk == 65536 else {'chunk': chunk}
            decoded = self.model.impute(torch.as_tensor(np.asarray(data)).float(), compose=[modality, to_modality], **kw)
        return np.array(self.model.preprocessing_inverse[to_modality](decoded.detach().cpu()))

    def impute(self, data, modality, pre_transformed=False, chunk=65536):
        """north_star spelling of `modal_predict`."""
        return self.modal_predict(data, modality, pre_transformed, chunk)

    def feature_impact(self, data, modality, to_modality=None, pre_transformed=False, background=None, features=None, measured=None,
                       max_workspace=1 << 30):
        """Occlusion impact of the input features of `modality` on the values imputed for `to_modality` (default: the next one, as in
        `modal_predict`): the mean squared change of the imputation, in the network's standardised output space, when ONE feature
        of every cell is set to its background value -- build-defined, see jamie_amd/impact.py.  Returns float64 numpy
        {'impact' [F], 'per_target' [F, d_to], 'baseline' [d_to] or None}.

        `pre_transformed=False`: the modality's fitted preprocessing must be per-feature standardisation (no PCA); `data` and
        `background` are in data units (`background` defaults to the fitted mean) and `measured`, if given, goes through the
        target modality's preprocessing.  `pre_transformed=True`: all three are in the network's own spaces and the features are
        the network's input columns -- the only spelling for a PCA'd modality.  `data` may be a scipy sparse matrix.  `measured`
        [cells, d_to]: the reference becomes the measured values and `baseline` is the un-occluded error.  `max_workspace`: cap in
        bytes on the widest activation of a pass."""
        from . import impact as jfi
        assert self.model is not None, 'Model must be trained before feature impact.'
        to_modality = (modality + 1) % self.dataset_num if to_modality is None else int(to_modality)
        model = self.model
        if not (0 <= int(modality) < self.dataset_num and 0 <= to_modality < self.dataset_num):
            raise ValueError(f'feature_impact: modalities must lie in [0, {self.dataset_num}), got {modality} and {to_modality}')
        if not pre_transformed:
            pre = self._csr_preclass(modality)
            if pre is None:
                raise ValueError(f'feature_impact: modality {modality} was not fitted with plain per-feature standardisation (a PCA, '
                                 'or a model class of the caller\'s), so its input features are not the data\'s; pass pre-processed '
                                 'cells with pre_transformed=True: the features are then the network\'s input columns')
            mean = np.asarray(pre.mean, dtype=np.float64).reshape(-1)
            if background is not None:
                background = np.asarray(background.cpu() if torch.is_tensor(background) else background, dtype=np.float64)
                if background.shape != mean.shape:
                    raise ValueError(f'feature_impact: background must be one value per feature [{mean.size}], got shape '
                                     f'{background.shape}')
                background = pre.transform(background)
            if measured is not None:
                measured = self.model.preprocessing[to_modality](np.asarray(measured.cpu() if torch.is_tensor(measured) else measured))
            if sp.issparse(data):
                jfi.check_arguments(model, data, modality, to_modality, background, features, measured, max_workspace)
                chunks = list(self._csr_chunks(data, modality, pre, 65536))
                data = torch.cat(chunks, 0) if len(chunks) > 1 else chunks[0]
            else:
                data = np.asarray(data.cpu() if torch.is_tensor(data) else data)
                if data.ndim != 2 or data.shape[1] != mean.size:
                    raise ValueError(f'feature_impact: cells must be 2-D [cells, {mean.size} features], got shape {data.shape}')
                data = pre.transform(data)
        elif sp.issparse(data):
            data = data.toarray()
        out = jfi.feature_impact(model, data, modality, to_modality, background=background, features=features, measured=measured,
                                 max_workspace=max_workspace)
        top = int(np.argmax(out['impact']))
        print(f"feature impact {modality} -> {to_modality}: {len(out['impact'])} features, mean {float(out['impact'].mean())}, "
              f"largest {float(out['impact'][top])} at position {top}")
        return out

    def shapley_values(self, data, modality, to_modality=None, pre_transformed=False, background=None, features=None, targets=None,
                       n_permutations=16, antithetic=True, seed=0, orders=None, return_values=False, max_workspace=1 << 30,
                       max_accumulator=1 << 30):
        """Shapley attributions of the input features of `modality` for the values imputed for `to_modality` (default: the next one,
        as in `modal_predict`), per cell, by permutation walks -- build-defined, see jamie_amd/shapley.py.  A feature that is absent
        from a coalition is set to its background value.  Returns float64 numpy {'values' [N, F, T] (None unless `return_values`),
        'mean_abs' [F, T], 'mean' [F, T], 'importance' [F], 'orders' [P, F] int32}, in the network's standardised output space.

        `features` (default: all) are the players and `targets` (default: all) the columns of the target modality; both must be
        distinct.  `n_permutations` orders of the players are drawn with np.random.default_rng(seed); with `antithetic` each is
        followed by its reverse (2 n_permutations walks in all); an explicit `orders` [P, F] array (permutations of range(F),
        positions in `features`) overrides both.  The preprocessing rules are `feature_impact`'s: with `pre_transformed=False` the
        modality's fitted preprocessing must be per-feature standardisation (no PCA) and `data` and `background` are in data units
        (`background` defaults to the fitted mean); with `pre_transformed=True` both are in the network's input space and the
        features are its input columns -- the only spelling for a PCA'd modality.  `data` may be a scipy sparse matrix.
        `max_workspace`, `max_accumulator`: caps in bytes on the widest activation of a pass and on the float64 contributions of a
        cell chunk."""
        from . import shapley as jsh
        assert self.model is not None, 'Model must be trained before Shapley values.'
        to_modality = (modality + 1) % self.dataset_num if to_modality is None else int(to_modality)
        model = self.model
        if not (0 <= int(modality) < self.dataset_num and 0 <= to_modality < self.dataset_num):
            raise ValueError(f'shapley_values: modalities must lie in [0, {self.dataset_num}), got {modality} and {to_modality}')
        d_i = int(model.input_dim[int(modality)])
        if orders is None:
            n_players = d_i if features is None else int(np.asarray(features).size)
            orders = jsh.draw_orders(n_players, n_permutations, antithetic, seed)
        kw = dict(background=None, features=features, targets=targets, orders=orders, max_workspace=max_workspace,
                  max_accumulator=max_accumulator, return_values=return_values)
        if not pre_transformed:
            pre = self._csr_preclass(modality)
            if pre is None:
                raise ValueError(f'shapley_values: modality {modality} was not fitted with plain per-feature standardisation (a PCA, '
                                 'or a model class of the caller\'s), so its input features are not the data\'s; pass pre-processed '
                                 'cells with pre_transformed=True: the features are then the network\'s input columns')
            mean = np.asarray(pre.mean, dtype=np.float64).reshape(-1)
            if background is not None:
                background = np.asarray(background.cpu() if torch.is_tensor(background) else background, dtype=np.float64)
                if background.shape != mean.shape:
                    raise ValueError(f'shapley_values: background must be one value per feature [{mean.size}], got shape '
                                     f'{background.shape}')
                background = pre.transform(background)
            kw['background'] = background
            if sp.issparse(data):
                jsh.check_arguments(model, data, modality, to_modality, **kw)
                chunks = list(self._csr_chunks(data, modality, pre, 65536))
                data = torch.cat(chunks, 0) if len(chunks) > 1 else chunks[0]
            else:
                data = np.asarray(data.cpu() if torch.is_tensor(data) else data)
                if data.ndim != 2 or data.shape[1] != mean.size:
                    raise ValueError(f'shapley_values: cells must be 2-D [cells, {mean.size} features], got shape {data.shape}')
                data = pre.transform(data)
        else:
            kw['background'] = background
            if sp.issparse(data):
                data = data.toarray()
        out = jsh.shapley_values(model, data, modality, to_modality, **kw)
        top = int(np.argmax(out['importance']))
        print(f"shapley values {modality} -> {to_modality}: {len(out['importance'])} features, {len(out['orders'])} orders, mean |value| "
              f"{float(out['importance'].mean())}, largest {float(out['importance'][top])} at position {top}")
        return out

    def transform(self, dataset, corr=None, pre_transformed=False, chunk=65536):
        """reference jamie.py:817-829.  In eval mode the returned embeddings are the `mu`s, so `corr` has no
        effect ("Doesn't actually do anything", jamie.py:820) and no N x N matrix is built.  A modality may be a scipy sparse
        matrix: its rows are streamed through the GPU `chunk` at a time (a modality fitted with an sklearn PCA, preprocess='host', is
        densified on the host)."""
        return [self._embed_input(d, i, pre_transformed, chunk).cpu().numpy() for i, d in enumerate(dataset)]

    def transform_one(self, data, i, pre_transformed=False, chunk=65536):
        """reference jamie.py:831-837; `data` may be a scipy sparse matrix (see `transform`)."""
        return self._embed_input(data, i, pre_transformed, chunk).cpu().numpy()

    # ------------------------------------------------------------------------------------------
    def save_model(self, f):
        """reference jamie.py:967-968.  Saved as state_dict + preprocessing objects (the reference's
        whole-module pickle no longer loads on torch >= 2.6)."""
        m = self.model
        torch.save({'format': 'jamie_amd.v1', 'input_dim': m.input_dim, 'output_dim': m.output_dim,
                    'dropout': m.dropout, 'state_dict': {k: v.cpu() for k, v in m.state_dict().items()},
                    'preprocessing': m.preprocessing, 'preprocessing_inverse': m.preprocessing_inverse}, f)

    def save_checkpoint(self, f, next_epoch, best_running_loss=np.inf, streak=0):
        """Full training state after `next_epoch` epochs: parameters, BatchNorm statistics, both Adam moments, the
        device step / RNG counters, the host sampler's RNG, the early-stop bookkeeping and the loss history.  Rank-local:
        in a distributed run with the sharded optimiser every rank calls `engine.flush(collective=True)` first (the training
        loop does), else this raises instead of starting collectives on one rank."""
        eng, m = self.engine, self.model
        eng.flush()
        torch.save({'format': 'jamie_amd.ckpt.v2', 'epoch': int(next_epoch), 'input_dim': list(m.input_dim),
                    'output_dim': m.output_dim, 'dropout': m.dropout, 'batch_size': eng.B,
                    'compute_dtype': eng.compute_dtype,
                    'state_dict': {k: v.cpu() for k, v in m.state_dict().items()},
                    'flat': m.flat.cpu(), 'exp_avg': eng.exp_avg.cpu(), 'exp_avg_sq': eng.exp_avg_sq.cpu(),
                    'engine_state': eng.state.cpu(), 'num_batches_tracked': int(m.num_batches_tracked),
                    'best_running_loss': float(best_running_loss), 'streak': int(streak),
                    'loss_history': {k: list(v) for k, v in self.loss_history.items()},
                    'np_random': np.random.get_state(), 'py_random': random.getstate()}, f)

    def _load_checkpoint(self, f, eng):
        ck = torch.load(f, weights_only=False)
        m = self.model
        if ck.get('format') == 'jamie_amd.ckpt.v1':
            raise ValueError(f'{f}: checkpoint format v1 (round 2) is not supported after the parameter-layout change of '
                             f'format v2 (the flat buffers are ordered differently); re-train, or load its state_dict with load_model')
        if ck.get('format') != 'jamie_amd.ckpt.v2':
            raise ValueError(f'{f}: not a jamie_amd training checkpoint')
        if list(ck['input_dim']) != list(m.input_dim) or ck['output_dim'] != m.output_dim or ck['batch_size'] != eng.B \
                or ck['compute_dtype'] != eng.compute_dtype:
            raise ValueError(f'{f}: checkpoint of a different configuration (features {ck["input_dim"]}, latent '
                             f'{ck["output_dim"]}, batch {ck["batch_size"]}, {ck["compute_dtype"]})')
        m.load_state_dict(ck['state_dict'])
        m.flat.copy_(ck['flat'])                       # incl. alignment padding: bit-identical continuation
        m.num_batches_tracked = ck['num_batches_tracked']
        eng.exp_avg.copy_(ck['exp_avg'])
        eng.exp_avg_sq.copy_(ck['exp_avg_sq'])
        eng.state[1:].copy_(ck['engine_state'][1:])    # step counters; the Philox seed stays this rank's own
        if eng.bf16:
            eng.refresh_weights_bf16()
        if self.record_loss:
            self.loss_history = {k: list(v) for k, v in ck['loss_history'].items()}
        np.random.set_state(ck['np_random'])
        random.setstate(ck['py_random'])
        return ck['epoch'], ck['best_running_loss'], ck['streak']

    def load_model(self, f):
        """reference jamie.py:970-972."""
        ck = torch.load(f, weights_only=False)
        m = self.model_class(ck['input_dim'], ck['output_dim'], preprocessing=ck['preprocessing'],
                             preprocessing_inverse=ck['preprocessing_inverse'], dropout=ck['dropout'])
        m.load_state_dict(ck['state_dict'])
        self.model = m.to(self.device)
        self.dataset_num = self.model.num_modalities

    # ---- acceptance metrics (reference jamie.py:892-915 and 943-961); metrics='device': jamie_amd/metrics.py ----
    def test_closer(self, integrated_data, distance_metric=None):
        """FOSCTTM: fraction of samples closer than the true match."""
        assert len(integrated_data) == 2, 'Two datasets are supported for FOSCTTM'
        if self.metrics == 'device':
            if distance_metric not in (None, 'euclidean'):
                raise ValueError(f"metrics='device' computes FOSCTTM on euclidean distances only, not {distance_metric!r}")
            from . import metrics as jmetrics
            foscttm = jmetrics.foscttm(integrated_data[0], integrated_data[1], device=self.device)
            print(f'foscttm: {foscttm}')
            return foscttm
        from sklearn.metrics.pairwise import pairwise_distances
        d = pairwise_distances(np.concatenate(integrated_data, axis=0), metric='euclidean')
        size = integrated_data[0].shape[0]
        closer = 0
        for i in range(size):
            ld = d[i][size:]
            closer += np.sum(ld < ld[i])
            ld = d[size + i][:size]
            closer += np.sum(ld < ld[i])
        foscttm = closer / (2 * size ** 2)
        print(f'foscttm: {foscttm}')
        return foscttm

    def test_LabelTA(self, integrated_data, datatype, k=5):
        """Label transfer accuracy: a k-nearest-neighbour classifier fitted on integrated_data[1] with datatype[1] predicts the
        labels of integrated_data[0]; its accuracy against datatype[0]."""
        if self.metrics == 'device':
            from . import metrics as jmetrics
            acc = jmetrics.label_transfer_accuracy(integrated_data[0], datatype[0], integrated_data[1], datatype[1], k=k,
                                                   device=self.device)
        else:
            from sklearn.neighbors import KNeighborsClassifier
            knn = KNeighborsClassifier(n_neighbors=k)
            knn.fit(_host_array(integrated_data[1]), np.asarray(datatype[1]))
            acc = float(np.mean(knn.predict(_host_array(integrated_data[0])) == np.asarray(datatype[0])))
        print(f'label transfer accuracy: {acc}')
        return acc

    def test_silhouette(self, integrated_data, datatype):
        """Silhouette widths of the pooled embeddings: by label (how well the cell types separate: `label_asw`, `label_widths`) and
        by modality within every label (how well the modalities mix: `modality_asw`, `modality_asw_per_label`, 1 - |s| averaged,
        NaN for a label present in fewer than two modalities), plus the label x label mean-distance matrix `label_distance` and the
        `labels` in `np.unique` order.  Needs neither paired cells nor equal cell counts.  metrics='host': sklearn in float64 on
        N x N distances; metrics='device': jamie_amd/metrics.py `silhouette`."""
        if len(integrated_data) != len(datatype):
            raise ValueError(f'test_silhouette: {len(integrated_data)} embeddings but {len(datatype)} label arrays')
        for m, (e, lab) in enumerate(zip(integrated_data, datatype)):
            if np.ndim(lab) != 1 or len(lab) != e.shape[0]:
                raise ValueError(f'test_silhouette: one label per cell, got {np.shape(lab)} for the {e.shape[0]} cells of '
                                 f'embedding {m}')
        if self.metrics == 'device':
            from . import metrics as jmetrics
            out = jmetrics.silhouette(integrated_data, datatype, device=self.device)
        else:
            out = _host_silhouette([_host_array(e) for e in integrated_data], [np.asarray(lab) for lab in datatype])
        print(f"label ASW: {out['label_asw']}")
        print(f"modality ASW: {out['modality_asw']}")
        return out

    def test_lisi(self, integrated_data, datatype=None, perplexity=30, n_neighbors=None):
        """Local inverse Simpson index of the pooled embeddings (Korsunsky et al. 2019): `ilisi` with the modality as category
        (how well the modalities mix around every cell: 1 to the number of modalities) and, with labels, `clisi` with the label as
        category (how pure the cell types stay: 1 is best), their `*_median` and `*_scaled` figures in [0, 1] (1 is best for
        both), `n_neighbors` (default min(int(3 perplexity), cells - 1), at most 128), `n_failed` (cells whose weights all
        underflowed, NaN) and the `labels` in `np.unique` order.  Needs neither paired cells nor equal cell counts.
        metrics='host': float64 numpy on N x N distances; metrics='device': jamie_amd/neighbors.py `lisi`."""
        from . import neighbors as jnb
        n_cells = [e.shape[0] for e in integrated_data]
        perplexity, k = jnb.check_perplexity(perplexity, n_neighbors, int(sum(n_cells)), 'test_lisi')
        jnb.pooled_codes(n_cells, datatype, 'test_lisi')
        if self.metrics == 'device':
            out = jnb.lisi(integrated_data, datatype, perplexity=perplexity, n_neighbors=k, device=self.device)
        else:
            out = _host_lisi([_host_array(e) for e in integrated_data], datatype, perplexity, k)
        print(f"iLISI (median): {out['ilisi_median']}")
        print(f"cLISI (median): {out['clisi_median']}")
        return out

    def neighbors(self, integrated_data, k=15, mode='distance'):
        """The kNN graph of the pooled embeddings: scipy CSR [cells, cells] with every cell's k nearest other cells (1 <= k <=
        min(cells - 1, 128)), nearest first, ties to the lower index; the distances as float64 (`mode='distance'`) or ones
        (`mode='connectivity'`).  metrics='host': float64 numpy on N x N distances; metrics='device': jamie_amd/neighbors.py
        `knn_graph`."""
        from . import neighbors as jnb
        if mode not in ('distance', 'connectivity'):
            raise ValueError(f"neighbors: mode must be 'distance' or 'connectivity', not {mode!r}")
        k = jnb.check_k(k, int(sum(e.shape[0] for e in integrated_data)), 'neighbors')
        if self.metrics == 'device':
            return jnb.knn_graph(integrated_data, k=k, mode=mode, device=self.device)
        return _host_neighbors([_host_array(e) for e in integrated_data], k, mode)

    def test_layout(self, integrated_data, layout, n_neighbors=15, return_ranks=False):
        """How well `layout` keeps the neighbourhoods of `integrated_data`: any two representations of the same cells, one array
        per modality each, pooled.  Two uses: an embedding against its 2-D picture (`tsne`, `umap`, `spectral`), and `jm.dataset`
        against the integrated embedding (how much of each modality's measured structure the integration keeps).  Returns
        `trustworthiness` and `continuity` at K = n_neighbors (sklearn's definition; 1 <= K < cells / 2, K <= 64), their
        `*_curve` over k = 1 .. K, the co-ranking curve `qnx`, `lcmc` and its argmax `k_best`, the per-cell terms
        `cell_trustworthiness` / `cell_continuity` (one array per modality, to colour the plot with), `n_neighbors`, `n_cells`
        and, with `return_ranks`, the rank arrays and the lists.  metrics='host': float64 numpy on N x N distances, for a few
        thousand cells; metrics='device': jamie_amd/coranking.py `neighborhood_preservation`."""
        from . import coranking as jcr
        n_cells = jcr.check_spaces(integrated_data, layout, 'test_layout')
        k = jcr.check_neighbors(n_neighbors, int(sum(n_cells)), 'test_layout')
        if self.metrics == 'device':
            out = jcr.neighborhood_preservation(integrated_data, layout, n_neighbors=k, device=self.device,
                                                return_ranks=return_ranks)
        else:
            out = _host_layout([_host_array(e) for e in integrated_data], [_host_array(e) for e in layout], k, return_ranks)
        print(f"trustworthiness: {out['trustworthiness']}")
        print(f"continuity: {out['continuity']}")
        return out

    def test_clustering(self, integrated_data, datatype=None, n_clusters=None, n_init=4, max_iter=300, tol=1e-4, seed=0, init=None):
        """k-means of the pooled embeddings and how well the clusters recover the labels: `clusters` (int32 ids,
        one array per embedding), `centers` [k, L], `inertia`, `n_iter`, `converged`, `sizes` [k], `n_empty`, `run` (the winning
        one of `n_init` k-means++ runs; `init` [k, L] replaces the seeding and forces one run), `modality_contingency` [k, M] and,
        with labels, `ari`, `nmi` (sklearn's adjusted_rand_score and normalized_mutual_info_score), `contingency` [k, T] and the
        `labels` in `np.unique` order (each None without labels).  `n_clusters` defaults to the number of distinct labels.
        metrics='host': float64 numpy, for a few thousand cells; metrics='device': jamie_amd/clustering.py `clustering`."""
        from . import clustering as jcl
        k, n_init, max_iter, tol, init = jcl.check_clustering(integrated_data, datatype, n_clusters, n_init, max_iter, tol, init,
                                                              'test_clustering')
        if self.metrics == 'device':
            out = jcl.clustering(integrated_data, datatype, n_clusters=k, n_init=n_init, max_iter=max_iter, tol=tol, seed=seed,
                                 init=init, device=self.device)
        else:
            out = _host_clustering([_host_array(e) for e in integrated_data], datatype, k, n_init, max_iter, tol, seed, init)
        print(f"ARI: {out['ari']}")
        print(f"NMI: {out['nmi']}")
        return out

    def tsne(self, integrated_data, perplexity=30, n_neighbors=None, n_iter=1000, early_exaggeration=12.0, exaggeration_iter=250,
             learning_rate='auto', init='pca', seed=0, log_every=50, seg_rows=0):
        """t-SNE layout of the pooled embeddings with the exact gradient: `layout` (one float32 [cells, 2] array
        per embedding), `kl`, `kl_history` and `grad_norm_history` at the iterations `logged_at` (the multiples of `log_every`
        below `n_iter`, and `n_iter`), `n_neighbors` (default min(int(3 perplexity), cells - 1), at most 128: a perplexity below
        43 with the default), `learning_rate` ('auto': max(cells / early_exaggeration / 4, 50)) and `n_iter`.  sklearn's schedule
        and gains; `init` 'pca', 'random' (from `seed`) or an array [cells, 2]; no recentring, no early stop.
        metrics='host': float64 numpy on N x N arrays, for a few thousand cells; metrics='device': jamie_amd/tsne.py `tsne`."""
        from . import tsne as jts
        seg_rows = jts._check_seg_rows(seg_rows, 'tsne')
        checked = jts.check_tsne(integrated_data, perplexity, n_neighbors, n_iter, early_exaggeration, exaggeration_iter,
                                 learning_rate, init, log_every, 'tsne')
        if self.metrics == 'device':
            out = jts.tsne_checked(integrated_data, *checked, seed, self.device, seg_rows)
        else:
            out = _host_tsne([_host_array(e) for e in integrated_data], *checked, seed)
        print(f"t-SNE KL divergence: {out['kl']}")
        return out

    def umap(self, integrated_data, n_neighbors=15, min_dist=0.1, spread=1.0, n_epochs=None, learning_rate=1.0,
             negative_sample_rate=5, repulsion_strength=1.0, init='pca', seed=0, a=None, b=None, return_graph=False):
        """UMAP layout of the pooled embeddings: `layout` (one float32 [cells, 2] array per embedding), the curve
        `a`, `b` (fitted to `min_dist` and `spread` unless given), `n_epochs` (default 500 up to 10 000 cells, else 200),
        `n_neighbors`, `n_edges` (stored entries of the fuzzy graph), `n_fired` (entries fired over all epochs) and `graph` (the
        fuzzy graph, scipy CSR float32, with `return_graph`; else None).  Synchronous epochs, exactly `negative_sample_rate` draws
        per firing, `init` 'pca', 'random' (from `seed`) or an array [cells, 2].
        metrics='host': float64 numpy on N x N arrays, for a few thousand cells; metrics='device': jamie_amd/umap.py `umap`."""
        from . import umap as jum
        checked = jum.check_umap(integrated_data, n_neighbors, min_dist, spread, n_epochs, learning_rate, negative_sample_rate,
                                 repulsion_strength, init, a, b, 'umap')
        if self.metrics == 'device':
            out = jum.umap_checked(integrated_data, *checked, seed, return_graph, self.device)
        else:
            out = _host_umap([_host_array(e) for e in integrated_data], *checked, seed, return_graph)
        print(f"UMAP: {out['n_edges']} edges, {out['n_fired']} firings over {out['n_epochs']} epochs")
        return out

    def spectral(self, integrated_data, n_components=2, n_neighbors=15, kind='laplacian', density_normalize=None, tol=1e-8,
                 max_iter=100, max_degree=60, seed=0, return_graph=False):
        """Spectral embedding of the pooled embeddings: the eigenvectors of the `n_components` + 1 largest
        eigenvalues of the normalised fuzzy graph of `umap` -- umap-learn's spectral layout (`kind='laplacian'`) or scanpy's
        diffusion map (`kind='diffmap'`, which turns `density_normalize` on unless it is given).  `vectors` (one float64 [cells,
        n_components + 1] array per embedding, the trivial vector first), `embedding` (the same without it), `eigenvalues`,
        `residuals`, `degree`, `umap_init` (float32 [cells, 2] for `umap(init=...)`), `converged`, `iterations`, `applies`,
        `degrees`, `n_neighbors`, `n_edges` and `graph` (scipy CSR with `return_graph`).  `spectral.pseudotime(out, root)` gives
        the diffusion pseudotime.  metrics='host': float64 numpy on N x N arrays and `numpy.linalg.eigh`, for a few thousand
        cells; metrics='device': jamie_amd/spectral.py `spectral`."""
        from . import spectral as jsp
        checked = jsp.check_spectral(integrated_data, n_components, n_neighbors, kind, density_normalize, tol, max_iter, max_degree,
                                     'spectral')
        if self.metrics == 'device':
            out = jsp.spectral_checked(integrated_data, *checked, seed, return_graph, self.device)
        else:
            out = _host_spectral([_host_array(e) for e in integrated_data], *checked, return_graph)
        print(f"spectral: eigenvalues {out['eigenvalues'][0]:.6f} .. {out['eigenvalues'][-1]:.6f}, largest residual "
              f"{out['residuals'].max():.2e}, {out['applies']} applies")
        return out

    def louvain(self, integrated_data, datatype=None, resolution=1.0, n_neighbors=15, max_levels=20, max_sweeps=32, tol=1e-7,
                return_graph=False):
        """Louvain communities of the pooled embeddings (scanpy's `tl.louvain`): multi-level modularity
        optimisation of the fuzzy graph of `umap` at `resolution`, with the weights as integers (val 2^20, rounded), so that every
        sum is exact and the result is the same bits on every run and on both routes for one graph.  `clusters` (int32 ids by
        descending size, one array per embedding: usable as `rank_features(..., labels=)`), `n_clusters`, `sizes`, `modularity`,
        `levels` (per accepted level: nodes, communities, sweeps, the moved count per sweep, modularity, two_m),
        `modality_contingency` [clusters, M] and, with labels, `ari`, `nmi`, `contingency` and the `labels` in `np.unique` order
        (each None without labels), `n_neighbors`, `n_edges` and `graph` (scipy CSR with `return_graph`).  No refinement step
        and no splitting of disconnected communities: that is `leiden`.  metrics='host': int64 / float64 numpy on N x N distances, for a
        few thousand cells; metrics='device': jamie_amd/louvain.py `louvain`."""
        from . import louvain as jlv
        checked = jlv.check_louvain(integrated_data, datatype, resolution, n_neighbors, max_levels, max_sweeps, tol, 'louvain')
        if self.metrics == 'device':
            out = jlv.louvain_checked(integrated_data, datatype, *checked, return_graph, self.device)
        else:
            out = _host_louvain([_host_array(e) for e in integrated_data], datatype, *checked, return_graph)
        print(f"louvain: {out['n_clusters']} clusters over {len(out['levels'])} levels, modularity {out['modularity']:.6f}, ARI "
              f"{out['ari']}")
        return out

    def leiden(self, integrated_data, datatype=None, resolution=1.0, n_neighbors=15, max_levels=20, max_sweeps=32, tol=1e-7,
               return_graph=False):
        """Leiden communities of the pooled embeddings (scanpy's `tl.leiden`; Traag, Waltman and van Eck 2019):
        per level Louvain's move phase on the integer fuzzy graph of `louvain`, then a refinement that splits every community
        into connected parts (only a node still alone joins a part, and only one inside its own community), then aggregation by
        the parts, each starting the next level in its community.  Deterministic: the merge takes the best part, not a random
        one.  The dict of `louvain`, with `levels` holding per level nodes, communities, sweeps, the moved count per sweep,
        modularity, refined (the parts: the next level's nodes), merged, cancelled and two_m (the last three None on a last level
        that was not refined), and `stop`: 'singletons' (no two nodes of the last level share a community), 'stuck' (no part
        would merge: the level's nodes are returned) or 'max_levels'.  Every returned community is connected in the graph unless
        stop is 'max_levels'.  `tol` is accepted for parity with `louvain` and unused.  The same bits on every run and on both
        routes for one graph.  metrics='host': int64 / float64 numpy on N x N distances, for a few thousand cells;
        metrics='device': jamie_amd/leiden.py `leiden`."""
        from . import louvain as jlv
        checked = jlv.check_louvain(integrated_data, datatype, resolution, n_neighbors, max_levels, max_sweeps, tol, 'leiden')
        if self.metrics == 'device':
            from . import leiden as jld
            out = jld.leiden_checked(integrated_data, datatype, *checked, return_graph, self.device)
        else:
            out = _host_leiden([_host_array(e) for e in integrated_data], datatype, *checked, return_graph)
        print(f"leiden: {out['n_clusters']} clusters over {len(out['levels'])} levels ({out['stop']}), modularity "
              f"{out['modularity']:.6f}, ARI {out['ari']}")
        return out

    def test_graph(self, integrated_data, datatype=None, n_neighbors=15, alpha=0.05, expected='global', return_graph=False):
        """Connected components, graph connectivity and kBET of the pooled embeddings on the fuzzy graph of `umap` (DESIGN.md
        §26; scIB's `graph_connectivity` and `kBET`).  `components` (int32 ids by descending size, one array per embedding),
        `n_components`, `component_sizes`, `largest_share`, `modality_contingency` [components, M], `label_contingency`, `rounds`
        and `jumps` of the min-label rounds; with labels `graph_connectivity` (the mean over labels of `label_connectivity` [T]:
        the share of a label's cells in the largest component of the graph cut down to that label), `label_components` [T] and the
        `labels` in `np.unique` order (each None without labels); with two or more embeddings `kbet_rejection` (the share of
        tested cells whose n_neighbors - 1 neighbours hold the modalities in other than the expected shares, chi-square at level
        `alpha`), `kbet_acceptance`, `kbet_pvalues` and `kbet_stat` per embedding (NaN where a cell is not tested), `kbet_tested`
        and `label_kbet_rejection` [T] (each None for a single embedding); `n_neighbors`, `n_edges`, `alpha`, `expected` and `graph`
        (scipy CSR with `return_graph`).  expected='global': the modality shares of the pooled cells; 'label': the shares among
        the cells of the cell's own label (build-defined).  No subsampling and no permutation null.  metrics='host': scipy's
        `connected_components` and float64 numpy on N x N distances, for a few thousand cells; metrics='device':
        jamie_amd/graph.py `graph_metrics`."""
        from . import graph as jgr
        checked = jgr.check_graph_metrics(integrated_data, datatype, n_neighbors, alpha, expected, 'test_graph')
        if self.metrics == 'device':
            out = jgr.graph_metrics_checked(integrated_data, datatype, *checked, return_graph, self.device)
        else:
            out = _host_test_graph([_host_array(e) for e in integrated_data], datatype, *checked, return_graph)
        print(f"test_graph: {out['n_components']} components (largest {out['largest_share']:.4f}), graph connectivity "
              f"{out['graph_connectivity']}, kBET rejection {out['kbet_rejection']}")
        return out

    def test_imputation(self, imputed, measured, threshold=0.0):
        """Per-feature imputation figures (reference evaluation.py): {'correlation', 'mse', 'auroc'}, float64 [features] each,
        between imputed values (`modal_predict`) and the measured ones.  AUROC scores the imputed value against `measured >
        threshold` (a scalar or one threshold per feature) and is NaN where a feature has one class; the correlation is NaN
        where a column is constant.  Prints the means over the features that have a figure."""
        if self.metrics == 'device':
            from . import imputation as jimp
            out = jimp.imputation_metrics(imputed, measured, threshold=threshold, device=self.device)
        else:
            dense = [x.toarray() if hasattr(x, 'toarray') else _host_array(x) for x in (imputed, measured)]
            out = _host_imputation_metrics(dense[0], dense[1], threshold)
        for name in ('correlation', 'mse', 'auroc'):
            v = out[name]
            mean = float(np.nanmean(v)) if np.any(~np.isnan(v)) else float('nan')
            print(f'imputation {name}: {mean}')
        return out

    def rank_features(self, data, labels, n_top=25, tie_correct=True, max_workspace=1 << 30):
        """Which features mark each group (scanpy's `rank_genes_groups`): every group of `labels` (cluster ids of
        `test_clustering`, or cell types) against the rest, for each feature of `data` [cells, features] -- measured values or
        what `modal_predict` imputes.  The dict of jamie_amd/markers.py `rank_features`: exact Wilcoxon rank sums (`rank_sum2`,
        `tie_term`, `U2`) with `auroc`, `z`, `pvals`, `pvals_adj`; `mean`, `var` and Welch's `t`, `t_df`, `t_pvals` of group
        against rest; `logfoldchanges` (assumes log1p data), `mean_difference`; `ranking` [groups, n_top] by descending `z`.  NaN
        where a statistic is undefined: a single group, a constant feature (`z`), fewer than 2 cells on a side (`var`, `t`).  At
        most 2^21 cells.  metrics='host': float64 numpy with `scipy.stats.rankdata` per feature; metrics='device':
        jamie_amd/markers.py (fp32 values, exact integer rank sums, fp64 moments)."""
        from . import markers as jmk
        N, d, labels, n_top = jmk.check_rank_features(data, labels, n_top)
        if self.metrics == 'device':
            out = jmk.rank_features(data, labels, n_top=n_top, tie_correct=tie_correct, max_workspace=max_workspace,
                                    device=self.device)
        else:
            out = _host_rank_features(data.toarray() if hasattr(data, 'toarray') else _host_array(data), labels, n_top, tie_correct)
        z = np.abs(out['z'])
        print(f"rank_features: {len(out['groups'])} groups, {d} features, largest |z| "
              f"{float(np.nanmax(z)) if np.any(~np.isnan(z)) else float('nan')}")
        return out


def _host_array(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def _host_silhouette(embeddings, labels):
    """The dict of `metrics.silhouette` in float64 with sklearn, on the N x N distance matrix of the pooled cells."""
    from sklearn.metrics import silhouette_samples
    from sklearn.metrics.pairwise import pairwise_distances
    M = len(embeddings)
    X = np.concatenate([np.asarray(e, dtype=np.float64) for e in embeddings], axis=0)
    lab = np.concatenate(labels)
    mod = np.repeat(np.arange(M), [len(e) for e in embeddings])
    classes, lcode = np.unique(lab, return_inverse=True)
    lcode = lcode.reshape(-1)
    T = len(classes)
    d = pairwise_distances(X, metric='euclidean')           # (raises ValueError on NaN / inf)
    widths = silhouette_samples(d, lcode, metric='precomputed')          # (ValueError unless 2 <= T <= N - 1)
    per_label = np.full(T, np.nan)
    for t in range(T):
        cells = np.nonzero(lcode == t)[0]
        mods = mod[cells]
        n_mod = len(np.unique(mods))
        if n_mod < 2:
            continue
        if n_mod < len(cells):
            s = silhouette_samples(d[np.ix_(cells, cells)], mods, metric='precomputed')
        else:
            s = np.zeros(len(cells))                        # every cell alone in its modality: sklearn's rule for singletons
        per_label[t] = float(np.mean(1.0 - np.abs(s)))
    have = ~np.isnan(per_label)
    onehot = (lcode[:, None] == np.arange(T)[None, :]).astype(np.float64)
    n = onehot.sum(axis=0)
    G = onehot.T @ d @ onehot                               # (d is symmetric; the two products need not round alike)
    return {'label_asw': float(np.mean(widths)), 'label_widths': widths,
            'modality_asw': float(np.mean(per_label[have])) if have.any() else float('nan'),
            'modality_asw_per_label': per_label,
            'label_distance': (G + G.T) / 2 / (n[:, None] * n[None, :]),
            'labels': classes}


def _host_sorted_neighbors(embeddings, k, what):
    """(idx int64 [N, k], dist float64 [N, k]) of the pooled cells on their N x N distance matrix: the diagonal at +inf, a stable
    argsort.  The distances are scipy's direct differences: sklearn's `pairwise_distances` expands |x|^2 + |y|^2 - 2 x.y, which
    loses the digits of close pairs and does not tie where the cells tie."""
    from scipy.spatial.distance import cdist
    if len(embeddings) < 1:
        raise ValueError(f'{what}: no embeddings')
    for e in embeddings:
        if e.ndim != 2 or e.shape[1] != embeddings[0].shape[1] or e.shape[1] < 1:
            raise ValueError(f'{what}: the embeddings must be [cells, features] with the same features')
    X = np.concatenate([np.asarray(e, dtype=np.float64) for e in embeddings], axis=0)
    if not np.isfinite(X).all():
        raise ValueError(f'{what}: input contains NaN or infinity')
    d = cdist(X, X)
    np.fill_diagonal(d, np.inf)
    order = np.argsort(d, axis=1, kind='stable')[:, :k]
    return order, np.take_along_axis(d, order, axis=1)


def _host_simpson(D, codes_nb, perplexity):
    """`compute_simpson_index` of the LISI package for one cell: its k distances D, its neighbours' category codes [n_sets, k].
    LISI per set (NaN where every weight underflowed)."""
    def hbeta(beta):
        P = np.exp(-D * beta)
        s = P.sum()
        if s == 0:
            return 0.0, np.zeros_like(D)
        return float(np.log(s) + beta * np.sum(D * P) / s), P / s
    log_u = np.log(perplexity)
    beta, bmin, bmax = 1.0, -np.inf, np.inf
    H, P = hbeta(beta)
    diff, tries = H - log_u, 0
    while abs(diff) > 1e-5 and tries < 50:
        if diff > 0:
            bmin = beta
            beta = beta * 2 if np.isinf(bmax) else (beta + bmax) / 2
        else:
            bmax = beta
            beta = beta / 2 if np.isinf(bmin) else (beta + bmin) / 2
        H, P = hbeta(beta)
        diff, tries = H - log_u, tries + 1
    if H == 0:
        return [np.nan] * len(codes_nb)
    return [1.0 / float(sum(P[c == b].sum() ** 2 for b in np.unique(c))) for c in codes_nb]


def _host_lisi(embeddings, labels, perplexity, k):
    """The dict of `neighbors.lisi` in float64 numpy, on the N x N distance matrix of the pooled cells."""
    from . import neighbors as jnb
    n_cells = [e.shape[0] for e in embeddings]
    mod, lcode, classes = jnb.pooled_codes(n_cells, labels, 'test_lisi')
    order, dist = _host_sorted_neighbors(embeddings, k, 'test_lisi')
    codes = [mod] if lcode is None else [mod, lcode]
    values = np.array([_host_simpson(dist[i], [c[order[i]] for c in codes], perplexity) for i in range(len(order))]).T
    return jnb.lisi_summary(values[0], None if lcode is None else values[1], len(embeddings), classes, k)


def _host_neighbors(embeddings, k, mode):
    """The CSR graph of `neighbors.knn_graph` in float64 numpy, on the N x N distance matrix of the pooled cells."""
    from . import neighbors as jnb
    order, dist = _host_sorted_neighbors(embeddings, k, 'neighbors')
    return jnb.graph_from_lists(order, dist, mode)


def _host_full_ranks(embeddings, what):
    """pos int32 [N, N] of the pooled cells: pos[i, j] = the 0-based rank of cell j among the other cells by (float64
    direct-difference distance to cell i, then lower index); N - 1 on the diagonal."""
    from scipy.spatial.distance import cdist
    for e in embeddings:
        if e.ndim != 2 or e.shape[1] != embeddings[0].shape[1] or e.shape[1] < 1:
            raise ValueError(f'{what}: the arrays of one space must be [cells, features] with the same features')
    X = np.concatenate([np.asarray(e, dtype=np.float64) for e in embeddings], axis=0)
    if not np.isfinite(X).all():
        raise ValueError(f'{what}: input contains NaN or infinity')
    d = cdist(X, X)
    np.fill_diagonal(d, np.inf)
    order = np.argsort(d, axis=1, kind='stable')
    pos = np.empty(order.shape, np.int32)
    np.put_along_axis(pos, order, np.arange(len(X), dtype=np.int32)[None, :], axis=1)
    return pos, order


def _host_layout(high, low, k, return_ranks=False):
    """The dict of `coranking.neighborhood_preservation` in float64 numpy, on the N x N distance matrices of both spaces."""
    from . import coranking as jcr
    n_cells = jcr.check_spaces(high, low, 'test_layout')
    pos_high, order_high = _host_full_ranks(high, 'test_layout')
    pos_low, order_low = _host_full_ranks(low, 'test_layout')
    idx_high, idx_low = order_high[:, :k], order_low[:, :k]
    rank_high = np.take_along_axis(pos_high, idx_low, axis=1)
    rank_low = np.take_along_axis(pos_low, idx_high, axis=1)
    out = jcr.preservation_summary(n_cells, k, jcr.host_rank_sums(rank_high), jcr.host_rank_sums(rank_low))
    if return_ranks:
        out.update(rank_high=rank_high, rank_low=rank_low, idx_high=idx_high.astype(np.int32), idx_low=idx_low.astype(np.int32))
    return out


def _host_affinities(dist, perplexity):
    """The conditional affinities of `tsne.affinities` in float64 numpy: (C [N, k], beta [N], tries [N]); sklearn's
    `_binary_search_perplexity` on e_j = d_j^2 - d_1^2."""
    from . import tsne as jts
    log_u = np.log(perplexity)
    N, k = dist.shape
    C, betas, tries = np.empty((N, k)), np.empty(N), np.empty(N, np.int32)
    for i in range(N):
        e = dist[i] ** 2 - dist[i, 0] ** 2
        beta, bmin, bmax, t = 1.0, -np.inf, np.inf, 0
        while True:
            P = np.exp(-beta * e)
            s = P.sum()
            diff = np.log(s) + beta * np.sum(e * P) / s - log_u
            if not (abs(diff) > jts.ENTROPY_TOL and t < jts.MAX_TRIES):
                break
            if diff > 0:
                bmin = beta
                beta = beta * 2 if np.isinf(bmax) else (beta + bmax) / 2
            else:
                bmax = beta
                beta = beta / 2 if np.isinf(bmin) else (beta + bmin) / 2
            t += 1
        C[i], betas[i], tries[i] = P / s, beta, t
    return C, betas, tries


def _host_joint(order, C):
    """P = (C + C^T) / (2N) as a dense float64 [N, N] matrix."""
    N = len(order)
    cond = np.zeros((N, N))
    np.put_along_axis(cond, order, C, axis=1)
    return (cond + cond.T) / (2.0 * N)


def _host_gradient(P, Y, alpha):
    """(grad [N, 2], Z, KL) of DESIGN.md §19 in float64 on N x N arrays."""
    from scipy.spatial.distance import cdist
    W = 1.0 / (1.0 + cdist(Y, Y, 'sqeuclidean'))
    np.fill_diagonal(W, 0.0)
    Z = float(W.sum())
    PW, W2 = P * W, W * W
    A = PW.sum(axis=1)[:, None] * Y - PW @ Y
    R = W2.sum(axis=1)[:, None] * Y - W2 @ Y
    nz = P > 0
    kl = float(np.sum(P[nz] * np.log(P[nz] * Z / W[nz])))
    return 4.0 * (alpha * A - R / Z), Z, kl


def _host_tsne(embeddings, perplexity, k, n_iter, early_exaggeration, exaggeration_iter, learning_rate, init, log_every, seed):
    """The dict of `tsne.tsne` in float64 numpy on N x N arrays: the same definition from the same initial layout
    (the PCA init is taken of the cells rounded to fp32, which is what the device route holds)."""
    from . import tsne as jts
    n_cells = [e.shape[0] for e in embeddings]
    order, dist = _host_sorted_neighbors(embeddings, k, 'tsne')
    X = np.concatenate([np.asarray(e, dtype=np.float64) for e in embeddings], axis=0)
    C, _, _ = _host_affinities(dist, perplexity)
    P = _host_joint(order, C)
    Y = jts.initial_layout(X.astype(np.float32), init, seed).astype(np.float64)
    u, gain = np.zeros_like(Y), np.ones_like(Y)
    phases, logged_at = jts.schedule(n_iter, exaggeration_iter, early_exaggeration, log_every)
    kl_hist, gsq_hist = [], []
    for t, (alpha, momentum) in enumerate(phases):
        g, _, kl = _host_gradient(P, Y, alpha)
        if t in logged_at:
            kl_hist.append(kl)
            gsq_hist.append(float(np.sum(g * g)))
        gain = np.maximum(np.where(u * g < 0, gain + 0.2, gain * 0.8), 0.01)
        u = momentum * u - learning_rate * (gain * g)
        Y = Y + u
    g, _, kl = _host_gradient(P, Y, 1.0)
    kl_hist.append(kl)
    gsq_hist.append(float(np.sum(g * g)))
    return jts.tsne_summary(Y, n_cells, kl_hist, gsq_hist, logged_at, k, learning_rate, n_iter)


def _host_smooth_knn(dist, n_neighbors):
    """`umap.smooth_knn` in float64 numpy: (W float32 [N, k], rho [N], sigma [N], tries [N]); umap-learn's `smooth_knn_dist`
    bisection with the sigma floor of DESIGN.md §20."""
    from . import umap as jum
    dist = np.asarray(dist, dtype=np.float64)
    N, k = dist.shape
    target = jum.smooth_target(n_neighbors)
    W, rho, sigma, tries = np.empty((N, k), np.float32), np.empty(N), np.empty(N), np.empty(N, np.int32)
    for i in range(N):
        d = dist[i]
        pos = d[d > 0]
        r = float(pos.min()) if pos.size else 0.0
        e = d - r
        lo, hi, mid, t = 0.0, np.inf, 1.0, 0
        while t < jum.MAX_TRIES:
            s = float(np.sum(np.where(e > 0, np.exp(-np.maximum(e, 0.0) / mid), 1.0)))
            t += 1
            if abs(s - target) < jum.SUM_TOL:
                break
            if s > target:
                hi = mid
                mid = (lo + hi) / 2
            else:
                lo = mid
                mid = mid * 2 if np.isinf(hi) else (lo + hi) / 2
        sg = max(mid, jum.SIGMA_FLOOR * float(d.sum()) / n_neighbors)
        W[i] = np.where((e <= 0) | (sg == 0), 1.0, np.exp(-np.maximum(e, 0.0) / (sg if sg > 0 else 1.0)))
        rho[i], sigma[i], tries[i] = r, sg, t
    return W, rho, sigma, tries


def _host_fuzzy_graph(order, W):
    """A = W + W^T - W o W^T of the lists `order` [N, k] and their fp32 weights W as CSR arrays (rowptr int64, col int32, val
    float32) in the row order of DESIGN.md §20: a row's own k entries in neighbour order, then the cells that list it without
    being listed by it, ascending."""
    N, k = order.shape
    dense = np.zeros((N, N))
    listed = np.zeros((N, N), dtype=bool)
    np.put_along_axis(dense, order, np.asarray(W, dtype=np.float64), axis=1)
    np.put_along_axis(listed, order, True, axis=1)
    A = ((dense + dense.T) - dense * dense.T).astype(np.float32)
    rev = listed.T & ~listed
    cols = [np.concatenate([order[i], np.nonzero(rev[i])[0]]) for i in range(N)]
    rowptr = np.zeros(N + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum([len(c) for c in cols])
    col = np.concatenate(cols).astype(np.int32)
    row = np.repeat(np.arange(N), np.diff(rowptr))
    return rowptr, col, A[row, col]


def _host_umap_epoch(row, col, eps, nxt, Y, n, alpha, a, b, gamma, negative_sample_rate, seed):
    """Epoch n of DESIGN.md §20 in float64 on the layout Y [N, 2]: (the layout after it, the entries fired).  `nxt` (float32)
    advances in place; `row` is the row of every CSR entry."""
    from . import umap as jum
    N = len(Y)
    fire = nxt <= np.float32(n)
    nxt[fire] = nxt[fire] + eps[fire]
    e = np.nonzero(fire)[0]
    i, j = row[e], col[e]

    def powers(d):
        d2 = np.sum(d * d, axis=1)
        safe = np.where(d2 > 0, d2, 1.0)
        return d2, safe, safe ** b

    d = Y[i] - Y[j]
    d2, safe, p = powers(d)
    c = np.where(d2 > 0, -2.0 * a * b * (p / safe) / (1.0 + a * p), 0.0)
    move = 2.0 * np.clip(c[:, None] * d, -4.0, 4.0)
    cells = jum.negative_cells(seed, e, n, negative_sample_rate, N)
    for r in range(negative_sample_rate):
        k = cells[:, r]
        d = Y[i] - Y[k]
        d2, safe, p = powers(d)
        c = np.where((d2 > 0) & (k != i), 2.0 * gamma * b / ((0.001 + safe) * (1.0 + a * p)), 0.0)
        move += np.clip(c[:, None] * d, -4.0, 4.0)
    delta = np.stack([np.bincount(i, weights=move[:, 0], minlength=N), np.bincount(i, weights=move[:, 1], minlength=N)], axis=1)
    return Y + alpha * delta, len(e)


def _host_umap(embeddings, n_neighbors, n_epochs, learning_rate, negative_sample_rate, repulsion_strength, init, a, b, seed,
               return_graph=False):
    """The dict of `umap.umap` in float64 numpy on N x N arrays: the same definition with the same draws, the
    same fp32 schedule, the same a, b and the same initial layout (the PCA init is taken of the cells rounded to fp32, which is
    what the device route holds)."""
    from . import umap as jum
    n_cells = [e.shape[0] for e in embeddings]
    order, dist = _host_sorted_neighbors(embeddings, n_neighbors - 1, 'umap')
    X = np.concatenate([np.asarray(e, dtype=np.float64) for e in embeddings], axis=0)
    W, _, _, _ = _host_smooth_knn(dist, n_neighbors)
    rowptr, col, val = _host_fuzzy_graph(order, W)
    row = np.repeat(np.arange(len(X)), np.diff(rowptr))
    eps, nxt = jum.schedule_arrays(val, n_epochs)
    Y = jum.initial_layout(X.astype(np.float32), init, seed).astype(np.float64)
    a32, b32 = jum.curve32(a, b)
    n_fired = 0
    for n in range(n_epochs):
        Y, fired = _host_umap_epoch(row, col, eps, nxt, Y, n, jum.alpha_of(learning_rate, n, n_epochs), a32, b32, repulsion_strength,
                                    negative_sample_rate, seed)
        n_fired += fired
    graph = None
    if return_graph:
        from scipy.sparse import csr_matrix
        graph = csr_matrix((val, col, rowptr), shape=(len(X), len(X)))
    return jum.umap_summary(Y, n_cells, a, b, n_epochs, n_neighbors, len(col), n_fired, graph)


def _host_spectral(embeddings, n_components, n_neighbors, kind, density_normalize, tol, max_iter, max_degree, return_graph=False):
    """The dict of `spectral.spectral` in float64 numpy on N x N arrays: the same graph, degree and scale, then
    `numpy.linalg.eigh` of the dense S.  No iteration: `iterations` and `applies` are 0."""
    from . import spectral as jsp
    n_cells = [e.shape[0] for e in embeddings]
    order, dist = _host_sorted_neighbors(embeddings, n_neighbors - 1, 'spectral')
    N = len(order)
    W, _, _, _ = _host_smooth_knn(dist, n_neighbors)
    rowptr, col, val = _host_fuzzy_graph(order, W)
    A = np.zeros((N, N))
    A[np.repeat(np.arange(N), np.diff(rowptr)), col] = val.astype(np.float64)
    degree = A.sum(axis=1)
    jsp.check_degree(degree)
    if density_normalize:
        inv = 1.0 / degree
        degree = (A @ inv) * inv
        jsp.check_degree(degree)
        scale = inv / np.sqrt(degree)
    else:
        scale = 1.0 / np.sqrt(degree)
    S = scale[:, None] * A * scale[None, :]
    k = n_components + 1
    w, V = np.linalg.eigh((S + S.T) / 2.0)
    theta, Q = w[::-1][:k].copy(), np.ascontiguousarray(V[:, ::-1][:, :k])
    resid = np.linalg.norm(S @ Q - Q * theta[None, :], axis=0)
    graph = None
    if return_graph:
        from scipy.sparse import csr_matrix
        graph = csr_matrix((val, col, rowptr), shape=(N, N))
    return jsp.spectral_summary(Q, theta, resid, degree, n_cells, resid.max() <= tol, 0, 0, [], n_neighbors, len(col), kind, density_normalize, tol,
                                graph)


def _host_louvain_move(rowptr, col, w, k, comm, tot, size, nodes, gamma, two_m):
    """The targets of `nodes` (int64 ids) from comm, tot and size as they stand, all rows at once: the
    entries are sorted by (node, community), summed per pair in int64 and the admitted pairs ordered by (node, gain descending,
    community ascending)."""
    lens = rowptr[nodes + 1] - rowptr[nodes]
    r = np.repeat(np.arange(len(nodes)), lens)
    e = np.repeat(rowptr[nodes] - (np.cumsum(lens) - lens), lens) + np.arange(int(lens.sum()))
    c = comm[nodes]
    d, we = comm[col[e]], w[e]
    own = d == c[r]
    kic = np.zeros(len(nodes), np.int64)
    np.add.at(kic, r[own], we[own])
    ki = k[nodes]
    gki = gamma * ki.astype(np.float64)
    m2 = float(two_m)
    gain_c = kic.astype(np.float64) - (gki * (tot[c] - ki).astype(np.float64)) / m2
    target = c.copy()
    ro, do, wo = r[~own], d[~own], we[~own]
    if len(ro):
        order = np.lexsort((do, ro))
        ro, do, wo = ro[order], do[order], wo[order]
        starts = np.nonzero(np.concatenate([[True], (ro[1:] != ro[:-1]) | (do[1:] != do[:-1])]))[0]
        kid, rg, dg = np.add.reduceat(wo, starts), ro[starts], do[starts]
        gain = kid.astype(np.float64) - (gki[rg] * tot[dg].astype(np.float64)) / m2
        ok = (gain > gain_c[rg]) & ~((size[c[rg]] == 1) & (size[dg] == 1) & (dg > c[rg]))
        rg, dg, gain = rg[ok], dg[ok], gain[ok]
        if len(rg):
            best = np.lexsort((dg, -gain, rg))
            rg, dg = rg[best], dg[best]
            head = np.concatenate([[True], rg[1:] != rg[:-1]])
            target[rg[head]] = dg[head]
    return target


def _host_louvain_sweeps(rowptr, col, w, k, comm, tot, size, gamma, two_m, max_sweeps):
    """The sweeps of a level on comm, tot and size in place: the moved count of every sweep."""
    from . import louvain as jlv
    cls = jlv.node_class(np.arange(len(k)))
    lists = [np.nonzero(cls == s)[0] for s in range(jlv.CLASSES)]
    history = []
    for _ in range(max_sweeps):
        moved = 0
        for nodes in lists:
            if not len(nodes):
                continue
            target = _host_louvain_move(rowptr, col, w, k, comm, tot, size, nodes, gamma, two_m)
            mv = target != comm[nodes]
            i, c, d = nodes[mv], comm[nodes][mv], target[mv]
            np.subtract.at(tot, c, k[i])
            np.add.at(tot, d, k[i])
            np.subtract.at(size, c, 1)
            np.add.at(size, d, 1)
            comm[i] = d
            moved += int(mv.sum())
        history.append(moved)
        if moved == 0 or jlv.stalled(history):
            break
    return history


def _host_louvain_inside(row, col, w, loop, comm):
    """in_c int64 [n] and the mask of the stored entries with both ends in one community."""
    inside_e = comm[row] == comm[col]
    inside = np.zeros(len(loop), np.int64)
    np.add.at(inside, comm, loop)
    np.add.at(inside, comm[row][inside_e], w[inside_e])
    return inside, inside_e


def _host_louvain_aggregate(row, col, w, loop, k, comm):
    """The next level's (rowptr, col, w, loop, k) and the new id of every node: communities renumbered in ascending id."""
    ids, cmap = np.unique(comm, return_inverse=True)
    cmap = cmap.reshape(-1)
    nc = len(ids)
    crow, ccol = cmap[row], cmap[col]
    inside_e = crow == ccol
    new_loop = np.zeros(nc, np.int64)
    np.add.at(new_loop, cmap, loop)
    np.add.at(new_loop, crow[inside_e], w[inside_e])
    keys, inv = np.unique(crow[~inside_e] * nc + ccol[~inside_e], return_inverse=True)
    new_w = np.zeros(len(keys), np.int64)
    np.add.at(new_w, inv.reshape(-1), w[~inside_e])
    new_k = np.zeros(nc, np.int64)
    np.add.at(new_k, cmap, k)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(keys // nc, minlength=nc))]).astype(np.int64)
    return rowptr, keys % nc, new_w, new_loop, new_k, cmap


def _host_louvain_levels(rowptr, col, w, loop, resolution=1.0, max_levels=20, max_sweeps=32, tol=1e-7):
    """DESIGN.md §23 on an integer level graph (rowptr, col, w int64, loop int64) in numpy: dict(comm int64 [n] the composed map
    of the accepted levels, modularity, levels)."""
    from . import louvain as jlv
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    w, loop = np.asarray(w, np.int64), np.asarray(loop, np.int64)
    n = len(loop)
    row = np.repeat(np.arange(n), np.diff(rowptr))
    k = loop.copy()
    np.add.at(k, row, w)
    two_m = int(k.sum())
    jlv.check_totals(n, two_m)
    q_prev = jlv.modularity_from_tables(loop, k, two_m, resolution)
    result = np.arange(n)
    levels = []
    while len(levels) < max_levels:
        n = len(loop)
        comm, tot, size = np.arange(n), k.copy(), np.ones(n, np.int64)
        history = _host_louvain_sweeps(rowptr, col, w, k, comm, tot, size, resolution, two_m, max_sweeps)
        inside, _ = _host_louvain_inside(row, col, w, loop, comm)
        q = jlv.modularity_from_tables(inside, tot, two_m, resolution)
        if not q > q_prev + tol:
            break
        rowptr, col, w, loop, k, cmap = _host_louvain_aggregate(row, col, w, loop, k, comm)
        row = np.repeat(np.arange(len(loop)), np.diff(rowptr))
        levels.append(jlv.level_record(n, len(loop), history, q, int(k.sum())))
        result = cmap[result]
        q_prev = q
    return dict(comm=result, modularity=q_prev, levels=levels)


def _host_louvain_graph(rowptr, col, val, resolution=1.0, max_levels=20, max_sweeps=32, tol=1e-7):
    """`louvain.communities` in numpy on the CSR arrays of any fp32 graph: dict(clusters int32 [N], sizes, modularity, levels)."""
    from . import louvain as jlv
    n = len(rowptr) - 1
    out = _host_louvain_levels(rowptr, col, jlv.quantise(val), np.zeros(n, np.int64), resolution, max_levels, max_sweeps, tol)
    clusters, sizes = jlv.relabel(out['comm'])
    return dict(clusters=clusters, sizes=sizes, modularity=out['modularity'], levels=out['levels'])


def _host_louvain(embeddings, labels, resolution, n_neighbors, max_levels, max_sweeps, tol, return_graph=False):
    """The dict of `louvain.louvain` in int64 / float64 numpy on `_host_fuzzy_graph`'s graph: the same definition."""
    from . import louvain as jlv
    n_cells = [e.shape[0] for e in embeddings]
    order, dist = _host_sorted_neighbors(embeddings, n_neighbors - 1, 'louvain')
    W, _, _, _ = _host_smooth_knn(dist, n_neighbors)
    rowptr, col, val = _host_fuzzy_graph(order, W)
    out = _host_louvain_graph(rowptr, col, val, resolution, max_levels, max_sweeps, tol)
    table_mod, table_lab, classes = jlv.host_tables(out['clusters'], n_cells, labels, len(out['sizes']))
    graph = None
    if return_graph:
        from scipy.sparse import csr_matrix
        graph = csr_matrix((val, col, rowptr), shape=(len(order), len(order)))
    return jlv.louvain_summary(out['clusters'], out['sizes'], out['modularity'], out['levels'], n_cells, table_mod, table_lab, classes,
                               resolution, n_neighbors, len(col), graph)


def _host_leiden_well(x, t, T, gamma, two_m):
    """wc(x, t) of DESIGN.md §24 on int64 arrays: (double)x >= ((gamma (double)t) (double)(T - t)) / (double)two_m."""
    return x.astype(np.float64) >= ((gamma * t.astype(np.float64)) * (T - t).astype(np.float64)) / float(two_m)


def _host_leiden_targets(rowptr, col, w, k, comm, tot, ref, rtot, rsize, cut, nodes, gamma, two_m):
    """The targets of `nodes` (int64 ids of one class) from the state as it stands, all rows at once: a
    node that is no longer alone keeps ref; for the others the entries inside the community are sorted by (node, part), summed per
    pair in int64 and the admitted pairs ordered by (node, gain descending, part ascending)."""
    target = ref[nodes].copy()
    alone = nodes[rsize[ref[nodes]] == 1]
    if not len(alone):
        return target
    lens = rowptr[alone + 1] - rowptr[alone]
    r = np.repeat(np.arange(len(alone)), lens)
    e = np.repeat(rowptr[alone] - (np.cumsum(lens) - lens), lens) + np.arange(int(lens.sum()))
    keep = comm[col[e]] == comm[alone][r]
    r, s, we = r[keep], ref[col[e[keep]]], w[e[keep]]
    cut_i = np.zeros(len(alone), np.int64)
    np.add.at(cut_i, r, we)
    ki, T = k[alone], tot[comm[alone]]
    well = _host_leiden_well(cut_i, ki, T, gamma, two_m)
    if not len(r):
        return target
    order = np.lexsort((s, r))
    r, s, we = r[order], s[order], we[order]
    starts = np.nonzero(np.concatenate([[True], (r[1:] != r[:-1]) | (s[1:] != s[:-1])]))[0]
    kis, rg, sg = np.add.reduceat(we, starts), r[starts], s[starts]
    gain = kis.astype(np.float64) - ((gamma * ki[rg].astype(np.float64)) * rtot[sg].astype(np.float64)) / float(two_m)
    ok = well[rg] & ~((rsize[sg] == 1) & (sg > alone[rg])) & _host_leiden_well(cut[sg], rtot[sg], T[rg], gamma, two_m) & (gain > 0.0)
    rg, sg, gain = rg[ok], sg[ok], gain[ok]
    if len(rg):
        best = np.lexsort((sg, -gain, rg))
        rg, sg = rg[best], sg[best]
        head = np.concatenate([[True], rg[1:] != rg[:-1]])
        at = np.searchsorted(nodes, alone[rg[head]])             # (`nodes` ascends)
        target[at] = sg[head]
    return target


def _host_leiden_refine(rowptr, col, w, k, comm, tot, gamma, two_m, trace=None):
    """DESIGN.md §24 step 3 on the communities comm of a level: (ref, merged, cancelled).  `trace` (a list) receives, per sub-sweep,
    ref and cut and the two counts so far."""
    from . import louvain as jlv
    n = len(k)
    row = np.repeat(np.arange(n), np.diff(rowptr))
    same = comm[row] == comm[col]
    cls = jlv.node_class(np.arange(n))
    ref, rtot, rsize = np.arange(n), k.copy(), np.ones(n, np.int64)
    merged = cancelled = 0
    for s in range(jlv.CLASSES):
        nodes = np.nonzero(cls == s)[0]
        target = ref.copy()
        leaves = same & (ref[row] != ref[col])
        cut = np.zeros(n, np.int64)
        np.add.at(cut, ref[row][leaves], w[leaves])
        if len(nodes):
            target[nodes] = _host_leiden_targets(rowptr, col, w, k, comm, tot, ref, rtot, rsize, cut, nodes, gamma, two_m)
            mv = target[nodes] != ref[nodes]
            i, d = nodes[mv], target[nodes][mv]
            stays = target[d] == d
            cancelled += int((~stays).sum())
            i, d = i[stays], d[stays]
            np.subtract.at(rtot, ref[i], k[i])
            np.add.at(rtot, d, k[i])
            np.subtract.at(rsize, ref[i], 1)
            np.add.at(rsize, d, 1)
            ref[i] = d
            merged += len(i)
        if trace is not None:
            trace.append(dict(ref=ref.copy(), cut=cut, merged=merged, cancelled=cancelled))
    return ref, merged, cancelled


def _host_leiden_levels(rowptr, col, w, loop, resolution=1.0, max_levels=20, max_sweeps=32, trace=None):
    """DESIGN.md §24 on an integer level graph (rowptr, col, w int64, loop int64) in numpy: dict(comm int64 [n] the returned
    partition composed down to the level-0 nodes, modularity, levels, stop).  `trace` (a list) receives one list per refined
    level (`_host_leiden_refine`)."""
    from . import leiden as jld
    from . import louvain as jlv
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    w, loop = np.asarray(w, np.int64), np.asarray(loop, np.int64)
    n = len(loop)
    row = np.repeat(np.arange(n), np.diff(rowptr))
    k = loop.copy()
    np.add.at(k, row, w)
    two_m = int(k.sum())
    jlv.check_totals(n, two_m, 'leiden')
    cells = np.arange(n)
    comm0, levels = np.arange(n), []
    while True:
        n = len(loop)
        comm, tot, size = comm0.copy(), np.zeros(n, np.int64), np.bincount(comm0, minlength=n).astype(np.int64)
        np.add.at(tot, comm, k)
        history = _host_louvain_sweeps(rowptr, col, w, k, comm, tot, size, resolution, two_m, max_sweeps)
        inside, _ = _host_louvain_inside(row, col, w, loop, comm)
        q = jlv.modularity_from_tables(inside, tot, two_m, resolution)
        nc = int((size > 0).sum())
        if nc == n or len(levels) + 1 >= max_levels:
            levels.append(jld.level_record(n, nc, history, q, two_m))
            return dict(comm=comm[cells], modularity=q, levels=levels, stop='singletons' if nc == n else 'max_levels')
        sub = None
        if trace is not None:
            sub = []
            trace.append(sub)
        ref, merged, cancelled = _host_leiden_refine(rowptr, col, w, k, comm, tot, resolution, two_m, sub)
        if merged == 0:
            levels.append(jld.level_record(n, nc, history, q, two_m, n, 0, cancelled))
            return dict(comm=cells, modularity=jlv.modularity_from_tables(loop, k, two_m, resolution), levels=levels, stop='stuck')
        rowptr, col, w, loop, k, cmap = _host_louvain_aggregate(row, col, w, loop, k, ref)
        row = np.repeat(np.arange(len(loop)), np.diff(rowptr))
        levels.append(jld.level_record(n, nc, history, q, two_m, len(loop), merged, cancelled))
        low = np.full(n, len(loop), np.int64)
        np.minimum.at(low, comm, cmap)
        comm0 = np.empty(len(loop), np.int64)
        comm0[cmap] = low[comm]
        cells = cmap[cells]


def _host_leiden_graph(rowptr, col, val, resolution=1.0, max_levels=20, max_sweeps=32, tol=1e-7, trace=None):
    """`leiden.communities` in numpy on the CSR arrays of any fp32 graph: dict(clusters int32 [N], sizes, modularity, levels,
    stop).  `tol` is unused."""
    from . import louvain as jlv
    n = len(rowptr) - 1
    out = _host_leiden_levels(rowptr, col, jlv.quantise(val), np.zeros(n, np.int64), resolution, max_levels, max_sweeps, trace)
    clusters, sizes = jlv.relabel(out['comm'])
    return dict(clusters=clusters, sizes=sizes, modularity=out['modularity'], levels=out['levels'], stop=out['stop'])


def _host_leiden(embeddings, labels, resolution, n_neighbors, max_levels, max_sweeps, tol, return_graph=False):
    """The dict of `leiden.leiden` in int64 / float64 numpy on `_host_fuzzy_graph`'s graph: the same definition."""
    from . import leiden as jld
    from . import louvain as jlv
    n_cells = [e.shape[0] for e in embeddings]
    order, dist = _host_sorted_neighbors(embeddings, n_neighbors - 1, 'leiden')
    W, _, _, _ = _host_smooth_knn(dist, n_neighbors)
    rowptr, col, val = _host_fuzzy_graph(order, W)
    out = _host_leiden_graph(rowptr, col, val, resolution, max_levels, max_sweeps, tol)
    table_mod, table_lab, classes = jlv.host_tables(out['clusters'], n_cells, labels, len(out['sizes']))
    graph = None
    if return_graph:
        from scipy.sparse import csr_matrix
        graph = csr_matrix((val, col, rowptr), shape=(len(order), len(order)))
    return jld.leiden_summary(out, n_cells, table_mod, table_lab, classes, resolution, n_neighbors, len(col), graph)


def _host_components(rowptr, col, n, cells=None):
    """The smallest member of every node's component (int32 [n]) by scipy's `connected_components` (weak); `cells`: the nodes of
    the induced subgraph to look at (their entries in the result; the other entries are -1)."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    A = csr_matrix((np.ones(len(col), np.int8), np.asarray(col), np.asarray(rowptr)), shape=(n, n))
    cells = np.arange(n) if cells is None else np.asarray(cells)
    _, lab = connected_components(A[cells][:, cells], directed=True, connection='weak')
    first = np.full(lab.max() + 1, n, dtype=np.int64)
    np.minimum.at(first, lab, cells)
    out = np.full(n, -1, dtype=np.int32)
    out[cells] = first[lab]
    return out


def _host_kbet(order, codes, shares, erow):
    """`jamie_kbet_stat` in float64 numpy: (stat [N], df [N], counts [N, B]) from `np.bincount` counts, the sum taken category
    after category in ascending order."""
    N, B = len(order), shares.shape[1]
    counts = np.stack([np.bincount(codes[order[i]], minlength=B) for i in range(N)]).astype(np.int64)
    f = shares[np.zeros(N, np.int64) if erow is None else erow]
    k = counts.sum(axis=1).astype(np.float64)
    stat, cats = np.zeros(N), np.zeros(N, np.int64)
    with np.errstate(invalid='ignore', divide='ignore'):
        for b in range(B):
            e = k * f[:, b]
            d = counts[:, b] - e
            have = f[:, b] > 0
            stat = np.where(have, stat + (d * d) / e, stat)
            cats += have
    tested = (k > 0) & (cats >= 2) & ~((counts > 0) & ~(f > 0)).any(axis=1)
    return np.where(tested, stat, np.nan), np.where(tested, cats - 1, 0).astype(np.int32), counts


def _host_test_graph(embeddings, labels, n_neighbors, alpha, expected, return_graph=False):
    """The dict of `graph.graph_metrics` on `_host_fuzzy_graph`'s graph: the components by scipy (per label on the induced
    subgraph), the round counts by the numpy rounds, kBET in float64 numpy: the same definition."""
    from . import graph as jgr
    from . import neighbors as jnb
    n_cells = [e.shape[0] for e in embeddings]
    mod, lcode, classes = jnb.pooled_codes(n_cells, labels, 'test_graph')
    order, dist = _host_sorted_neighbors(embeddings, n_neighbors - 1, 'test_graph')
    W, _, _, _ = _host_smooth_knn(dist, n_neighbors)
    rowptr, col, val = _host_fuzzy_graph(order, W)
    N = len(order)
    label = _host_components(rowptr, col, N)
    _, rounds, jumps = jgr.host_rounds(rowptr, col, N)
    share = count = None
    if lcode is not None:
        glabel = np.full(N, -1, dtype=np.int32)
        for t in range(len(classes)):
            cells = np.nonzero(lcode == t)[0]
            glabel[cells] = _host_components(rowptr, col, N, cells)[cells]
        share, count = jgr.label_connectivity(glabel, lcode, len(classes))
    kbet = None
    if len(embeddings) > 1:
        shares, erow = jgr.expected_rows(mod, len(embeddings), lcode, None if classes is None else len(classes), expected)
        stat, df, _ = _host_kbet(order, mod, shares, erow)
        kbet = dict(stat=stat, df=df)
    graph = None
    if return_graph:
        from scipy.sparse import csr_matrix
        graph = csr_matrix((val, col, rowptr), shape=(N, N))
    return jgr.graph_summary(label, rounds, jumps, n_cells, lcode, classes, share, count, kbet, n_neighbors, len(col), alpha, expected,
                             graph)


def _host_kmeans(X, k, n_init, max_iter, tol, seed, init):
    """The dict of `clustering.kmeans` in float64 numpy with float64 centres: the same definition, distances by
    direct difference (scipy's `cdist`: the expanded form loses the digits that decide between two near centres)."""
    from scipy.spatial.distance import cdist
    from . import clustering as jcl
    N, L = X.shape
    tol_abs = tol * float(np.mean(np.var(X, axis=0)))
    best = None
    for r in range(n_init):
        seeds = None
        if init is None:
            u = jcl.seeding_stream(seed, r, k)
            seeds = np.empty(k, np.int64)
            seeds[0] = min(int(u[0] * N), N - 1)
            minq = cdist(X, X[seeds[0]][None], 'sqeuclidean')[:, 0]
            for j in range(1, k):
                prefix = np.cumsum(minq)
                if prefix[-1] > 0:
                    seeds[j] = min(int(np.searchsorted(prefix, u[j] * prefix[-1], side='right')), N - 1)
                else:
                    seeds[j] = min(int(u[j] * N), N - 1)
                minq = np.minimum(minq, cdist(X, X[seeds[j]][None], 'sqeuclidean')[:, 0])
            C = X[seeds].copy()
        else:
            C = init.copy()
        prev, converged = None, False
        for t in range(1, max_iter + 1):
            q = cdist(X, C, 'sqeuclidean')
            lab = np.argmin(q, axis=1)                      # (the first minimum: ties to the lower centre)
            inertia = float(q[np.arange(N), lab].sum())
            counts = np.bincount(lab, minlength=k)
            sums = np.zeros((k, L))
            np.add.at(sums, lab, X)
            new = C.copy()
            new[counts > 0] = sums[counts > 0] / counts[counts > 0, None]
            shift = float(((new - C) ** 2).sum())
            same = prev is not None and np.array_equal(lab, prev)
            C, prev = new, lab
            if same or shift <= tol_abs:
                converged = True
                break
        if best is None or inertia < best['inertia']:
            best = {'labels': lab.astype(np.int32), 'centers': C, 'inertia': inertia, 'n_iter': t, 'converged': converged,
                    'sizes': counts.astype(np.int64), 'n_empty': int((counts == 0).sum()), 'run': r, 'seeds': seeds}
    return best


def _host_clustering(embeddings, labels, k, n_init, max_iter, tol, seed, init):
    """The dict of `clustering.clustering` in float64 numpy."""
    from . import clustering as jcl
    n_cells = [e.shape[0] for e in embeddings]
    mod, lcode, classes = jcl.pooled_codes(n_cells, labels, 'test_clustering')
    X = np.concatenate([np.asarray(e, dtype=np.float64) for e in embeddings], axis=0)
    km = _host_kmeans(X, k, n_init, max_iter, tol, seed, init)
    table_mod = np.zeros((k, len(embeddings)), np.int64)
    np.add.at(table_mod, (km['labels'], mod), 1)
    table_lab = None
    if lcode is not None:
        table_lab = np.zeros((k, len(classes)), np.int64)
        np.add.at(table_lab, (km['labels'], lcode), 1)
    return jcl.clustering_summary(km, n_cells, table_mod, table_lab, classes)


def _host_imputation_metrics(imputed, measured, threshold):
    """float64 numpy for the correlation and the MSE, sklearn's `roc_auc_score` per feature."""
    from sklearn.metrics import roc_auc_score
    X, Y = np.asarray(imputed, dtype=np.float64), np.asarray(measured, dtype=np.float64)
    if X.ndim != 2 or X.shape != Y.shape:
        raise ValueError(f'test_imputation: imputed and measured values must be [cells, features] of one shape, got {X.shape} '
                         f'and {Y.shape}')
    N, d = X.shape
    if N < 2 or d < 1:
        raise ValueError(f'test_imputation: N >= 2 cells and d >= 1 features are needed, got shape {X.shape}')
    if not (np.isfinite(X).all() and np.isfinite(Y).all()):
        raise ValueError('test_imputation: input contains NaN or infinity')
    thr = np.broadcast_to(np.asarray(threshold, dtype=np.float64), (d,))
    xc, yc = X - X.mean(0), Y - Y.mean(0)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = (xc * yc).sum(0) / np.sqrt((xc * xc).sum(0) * (yc * yc).sum(0))
    r[(np.ptp(X, axis=0) == 0) | (np.ptp(Y, axis=0) == 0)] = np.nan       # (centring a constant does not reliably leave 0)
    auroc = np.full(d, np.nan)
    for f in range(d):
        label = Y[:, f] > thr[f]
        if 0 < label.sum() < N:
            auroc[f] = roc_auc_score(label, X[:, f])
    return {'correlation': r, 'mse': ((X - Y) ** 2).mean(0), 'auroc': auroc}


def _host_rank_features(data, labels, n_top, tie_correct):
    """The dict of `markers.rank_features` in float64 numpy: midranks from `scipy.stats.rankdata` per feature, tie groups from
    `np.unique`, the same shifted sums as the device (pivot: row 0), finished by `markers.finish`."""
    from scipy.stats import rankdata
    from . import markers as jmk
    X = np.asarray(data, dtype=np.float64)
    N, d, labels, n_top = jmk.check_rank_features(X, labels, n_top)
    if not np.isfinite(X).all():
        raise ValueError('rank_features: input contains NaN or infinity')
    lay = jmk.group_layout(labels)
    starts = lay['seg_off'][:-1].astype(np.int64)
    Xs = X[lay['order']]                                                      # the cells in group order
    ranks2 = np.rint(2.0 * rankdata(Xs, axis=0)).astype(np.int64)            # (a midrank is a multiple of 1/2)
    rank_sum2 = np.add.reduceat(ranks2, starts, axis=0)
    tie_term = np.empty(d, np.int64)
    for f in range(d):
        t = np.unique(X[:, f], return_counts=True)[1].astype(object)          # (Python integers: t^3 up to 2^63)
        tie_term[f] = int((t ** 3 - t).sum())
    dx = Xs - X[0]
    sums = np.stack([np.add.reduceat(dx, starts, axis=0), np.add.reduceat(dx * dx, starts, axis=0)], axis=2)
    return jmk.finish(lay['groups'], lay['n'], rank_sum2, tie_term, X[0], sums, n_top, tie_correct)

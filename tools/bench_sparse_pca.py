"""Randomized PCA of sparse (CSR) cells on the device without a dense copy (jamie_amd/pca.py `SparseOperator`, csrc/sparse_pca.hip),
beside the dense `DevicePCA` on the densified matrix, on the same box and in the same process, the sparse route first.

    python tools/bench_sparse_pca.py [--shapes 100000x2000@0.05,100000x20000@0.05] [--k 50] [--reps 5] [--dense-max-gb 9]
                                     > profiles/bench_sparse_pca.log

Cells: `bench_sparse_input.make_cells` (1 + Poisson counts, per-gene storage probabilities log-normal: column lengths differ by
orders of magnitude).  Per shape and route, on resident inputs, HIP events around the call, one warm-up run, the median of --reps:
  right    Xc Q        [N, l], l = k + 10      sparse: jamie_weighted_colsum + jamie_csr_spmm on the CSR arrays; dense: NN GEMM
  left     Xc^T Y      [d, l]                  sparse: ... on the CSC arrays (row lengths = column lengths of X); dense: TN split-K
  scores   Xc V^T      [N, k]                  sparse: as `right` with k columns; dense: NT GEMM
then the whole `fit_transform_device` from the host matrix (wall time, upload and host algebra included, after the warm-up above) with
`torch.cuda.max_memory_allocated` over it.  Prints one line per shape and route and a JSON line at the end."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_sparse_input import make_cells, timed, wall  # noqa: E402
from jamie_amd import _native as nv  # noqa: E402
from jamie_amd import pca  # noqa: E402
from jamie_amd import sparse_input as jsp  # noqa: E402
from jamie_amd import sparse_pca as spp  # noqa: E402


def products(op, N, d, k, reps):
    """Median seconds of the three products of an operator, on random operands."""
    g = torch.Generator(device='cuda').manual_seed(1)
    ell = k + 10
    Q = torch.randn(d, ell, device='cuda', generator=g)
    Y = torch.randn(N, ell, device='cuda', generator=g)
    comp = torch.randn(k, d, device='cuda', generator=g)
    return {'right_s': timed(lambda: op.right(Q), reps)[0], 'left_s': timed(lambda: op.left(Y), reps)[0],
            'scores_s': timed(lambda: op.scores(comp), reps)[0]}


def fit(X, k):
    """(wall seconds, peak bytes above what was allocated before, the fitted DevicePCA) of one whole fit from the host matrix."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    dp = pca.DevicePCA(k, random_state=0)
    t, scores = wall(lambda: dp.fit_transform_device(X))
    peak = torch.cuda.max_memory_allocated() - before
    del scores
    return t, peak, dp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='100000x2000@0.05,100000x20000@0.05')
    ap.add_argument('--k', type=int, default=50)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--dense-max-gb', type=float, default=9.0)
    a = ap.parse_args()
    nv.require_gpu()
    prop = torch.cuda.get_device_properties(0)
    print(f'device: {prop.name}, {prop.multi_processor_count} CUs; k = {a.k} (l = {a.k + 10}); SEGMENT = {spp.SEGMENT}; fp32 values; '
          f'median of {a.reps} runs after a warm-up', flush=True)
    rows = []
    for spec in a.shapes.split(','):
        shape, density = spec.split('@')
        N, d = (int(v) for v in shape.split('x'))
        A = make_cells(N, d, float(density), torch.float32, N + d)
        nnz = int(A.nnz)
        lens = np.diff(A.tocsc().indptr)
        r = {'N': N, 'd': d, 'k': a.k, 'nnz': nnz, 'density': nnz / (N * d),
             'column_length_min_median_max': [int(lens.min()), float(np.median(lens)), int(lens.max())],
             'csr_plus_csc_bytes': 2 * nnz * 8 + 8 * (N + d + 2), 'dense_fp32_bytes': 4 * N * d}
        op = pca.SparseOperator(A, torch.device('cuda'))
        r['sparse'] = products(op, N, d, a.k, a.reps)
        del op
        t, peak, dp_s = fit(A, a.k)
        r['sparse'].update({'fit_wall_s': t, 'fit_peak_bytes': int(peak)})
        s = r['sparse']
        print(f"N={N} d={d} density {r['density']:.3f} (nnz {nnz}, column lengths {lens.min()} / {np.median(lens):.0f} / {lens.max()}) "
              f"sparse: right {s['right_s'] * 1e3:.3f} ms, left {s['left_s'] * 1e3:.3f} ms, scores {s['scores_s'] * 1e3:.3f} ms; whole fit "
              f"{t:.3f} s wall, peak {peak / 2 ** 20:.0f} MiB (CSR + CSC arrays {r['csr_plus_csc_bytes'] / 2 ** 20:.0f} MiB, a dense fp32 "
              f"copy {4 * N * d / 2 ** 20:.0f} MiB)", flush=True)
        if 4 * N * d <= a.dense_max_gb * 1e9:
            # the cells as a dense host array: the densify kernel against mean 0, sd 1 writes exactly them
            dense_host = jsp.apply_csr(A, np.zeros(d), np.ones(d)).cpu().numpy()
            torch.cuda.empty_cache()
            op = pca.DenseOperator(torch.from_numpy(dense_host).cuda())
            r['dense'] = products(op, N, d, a.k, a.reps)
            del op
            t, peak, dp_d = fit(torch.from_numpy(dense_host), a.k)
            r['dense'].update({'fit_wall_s': t, 'fit_peak_bytes': int(peak)})
            q = r['dense']
            r['max_relative_explained_variance_difference'] = float(np.max(np.abs(dp_s.explained_variance_ / dp_d.explained_variance_ - 1)))
            r['min_component_cosine'] = float(np.min(np.sum(dp_s.components_ * dp_d.components_, axis=1)))
            print(f"N={N} d={d} dense:  right {q['right_s'] * 1e3:.3f} ms, left {q['left_s'] * 1e3:.3f} ms, scores {q['scores_s'] * 1e3:.3f} ms; "
                  f"whole fit {t:.3f} s wall (host array of {dense_host.nbytes / 2 ** 20:.0f} MiB uploaded), peak {peak / 2 ** 20:.0f} MiB; "
                  f"sparse against dense fit: max relative explained-variance difference "
                  f"{r['max_relative_explained_variance_difference']:.2e}, smallest component cosine {r['min_component_cosine']:.6f}", flush=True)
            del dense_host
        else:
            print(f'N={N} d={d} dense:  skipped ({4 * N * d / 1e9:.1f} GB of dense fp32 above --dense-max-gb)', flush=True)
        rows.append(r)
        del A
        torch.cuda.empty_cache()
    print(json.dumps({'bench_sparse_pca': rows}))


if __name__ == '__main__':
    main()

"""Sparse (CSR) cell matrices on the device: per-feature statistics and the standardised dense fp32 matrix from the CSR arrays, beside
the dense route on the same cells.

    python tools/bench_sparse_input.py [--shapes 100000x2000@0.05,100000x2000@0.10,100000x20000@0.05,1000000x2000@0.05]
                                       [--reps 5] [--dtype f32] [--peak-tb 8.0] [--dense-max-gb 9]

Cells: 1 + Poisson(rate_c) at positions stored with probability p_c, p_c log-normal over the genes (sigma 2: column lengths differ
by orders of magnitude) and scaled to the density asked for; built on the GPU in row blocks and brought to the host as CSR arrays.
Per shape, on resident inputs, HIP events around the C-ABI calls, one warm-up run, the median of --reps runs:
  stats    jamie_csc_col_stats (CSC-ordered values + column pointers);
  densify  jamie_csr_standardise: time, the bytes it must move -- 4 N d written + nnz (value bytes + 4) + 8 N read -- over that time
           as a share of --peak-tb TB/s, and beside it the share of a device-to-device copy of 4 N d bytes (4 N d read + 4 N d
           written over its time), measured in the same run;
  dense    jamie_col_stats + jamie_standardise on the uploaded dense matrix (`_native.standardise_columns`).
Wall time from pageable host arrays to the resident standardised matrix, upload included, one run each after the kernels are warm:
`sparse_input.standardise_csr` on the scipy matrix (with the host's share of it: the canonical copy and `tocsc()`), and
`torch.from_numpy(dense).to(device)` + `standardise_columns` (skipped above --dense-max-gb of dense fp32).  Prints one line per shape and a
JSON line at the end."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jamie_amd import _native as nv  # noqa: E402
from jamie_amd import sparse_input as jsp  # noqa: E402


def timed(fn, reps):
    fn()                                                   # warm-up (code objects, allocator)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / 1e3)
    return statistics.median(ts), min(ts), max(ts)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def make_cells(N, d, density, dtype, seed):
    """scipy CSR [N, d] of 1 + Poisson counts with skewed per-gene storage probabilities, built on the GPU in row blocks."""
    g = torch.Generator(device='cuda').manual_seed(seed)
    p = torch.exp(2.0 * torch.randn(d, device='cuda', generator=g))
    for _ in range(30):                                     # scale to the density; probabilities saturate at 1
        p = torch.clamp(p * (density * d / p.sum()), max=1.0)
    rate = 0.5 + 4.0 * p
    block = max(1, min(N, (1 << 27) // d))
    counts, cols, vals = [], [], []
    for r0 in range(0, N, block):
        n = min(block, N - r0)
        mask = torch.rand(n, d, device='cuda', generator=g) < p
        counts.append(mask.sum(1).cpu().numpy())
        rc = mask.nonzero()
        v = 1.0 + torch.poisson(rate[rc[:, 1]], generator=g)
        cols.append(rc[:, 1].to(torch.int32).cpu().numpy())
        vals.append(v.to(dtype).cpu().numpy())
        del mask, rc, v
    indptr = np.concatenate([[0], np.cumsum(np.concatenate(counts))]).astype(np.int64)
    A = sp.csr_matrix((np.concatenate(vals), np.concatenate(cols), indptr), shape=(N, d))
    torch.cuda.empty_cache()
    return A


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='100000x2000@0.05,100000x2000@0.10,100000x20000@0.05,1000000x2000@0.05')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--dtype', default='f32', choices=['f32', 'f64'])
    ap.add_argument('--peak-tb', type=float, default=8.0, help="the MI355X's HBM bandwidth the shares are taken of, TB/s")
    ap.add_argument('--dense-max-gb', type=float, default=9.0)
    a = ap.parse_args()
    nv.require_gpu()
    prop = torch.cuda.get_device_properties(0)
    peak = a.peak_tb * 1e12
    tdt = torch.float32 if a.dtype == 'f32' else torch.float64
    vb = 4 if a.dtype == 'f32' else 8
    print(f'device: {prop.name}, {prop.multi_processor_count} CUs; shares are of {a.peak_tb} TB/s; SEGMENT = {jsp.SEGMENT}, WINDOW = '
          f'{jsp.WINDOW}, {a.dtype} values, median of {a.reps} runs after a warm-up')
    rows = []
    for spec in a.shapes.split(','):
        shape, density = spec.split('@')
        N, d = (int(v) for v in shape.split('x'))
        density = float(density)
        A = make_cells(N, d, density, tdt, N + d)
        nnz = A.nnz
        lens = np.diff(A.tocsc().indptr)
        # ---- resident inputs ----
        C = jsp.canonical_csr(A)
        csc = C.tocsc()
        p = jsp.plan(csc.indptr)
        cvals = torch.from_numpy(csc.data).cuda()
        colptr, seg_off = torch.from_numpy(csc.indptr.astype(np.int64)).cuda(), torch.from_numpy(p['seg_off']).cuda()
        del csc
        mean = torch.empty(d, dtype=torch.float64, device='cuda')
        sd = torch.empty(d, dtype=torch.float64, device='cuda')
        ws = torch.empty(p['workspace'], dtype=torch.uint8, device='cuda')
        t_stats = timed(lambda: nv.csc_col_stats(cvals, colptr, seg_off, p['segments'], N, mean, sd, ws), a.reps)
        del cvals, ws
        indptr, indices = torch.from_numpy(C.indptr).cuda(), torch.from_numpy(C.indices).cuda()
        vals = torch.from_numpy(C.data).cuda()
        del C
        out = torch.empty(N, d, dtype=torch.float32, device='cuda')
        wz = torch.empty(nv.sparse_workspace(None, d, 1), dtype=torch.uint8, device='cuda')
        t_dens = timed(lambda: nv.csr_standardise(indptr, indices, vals, d, mean, sd, out, wz), a.reps)
        dst = torch.empty_like(out)
        t_copy = timed(lambda: dst.copy_(out), a.reps)
        del dst, indptr, indices, vals
        moved = 4 * N * d + nnz * (vb + 4) + 8 * N
        r = {'N': N, 'd': d, 'density': nnz / (N * d), 'nnz': int(nnz), 'column_length_min_median_max': [int(lens.min()), float(np.median(lens)), int(lens.max())],
             'segments': p['segments'], 'stats_s': t_stats[0], 'stats_s_min_max': t_stats[1:], 'densify_s': t_dens[0],
             'densify_s_min_max': t_dens[1:], 'densify_bytes': moved, 'densify_share_of_peak': moved / t_dens[0] / peak,
             'copy_s': t_copy[0], 'copy_share_of_peak': 8 * N * d / t_copy[0] / peak}
        line = (f"N={N} d={d} density {r['density']:.3f} (nnz {nnz}, column lengths {lens.min()} / {np.median(lens):.0f} / {lens.max()}, "
                f"{p['segments']} segments): stats {t_stats[0] * 1e3:.3f} ms ({t_stats[1] * 1e3:.3f}-{t_stats[2] * 1e3:.3f}); densify "
                f"{t_dens[0] * 1e3:.3f} ms ({t_dens[1] * 1e3:.3f}-{t_dens[2] * 1e3:.3f}), {moved / t_dens[0] / 1e12:.2f} TB/s = "
                f"{r['densify_share_of_peak']:.2f} of peak (a copy of 4 N d bytes: {t_copy[0] * 1e3:.3f} ms = {r['copy_share_of_peak']:.2f})")
        # ---- wall time, sparse route (the kernels are warm) ----
        t_host, _ = wall(lambda: jsp.canonical_csr(A).tocsc())
        t_sparse, got = wall(lambda: jsp.standardise_csr(A))
        same = bool(torch.equal(got[0], out))
        r.update({'sparse_wall_s': t_sparse, 'sparse_wall_host_canonical_tocsc_s': t_host, 'sparse_upload_bytes': nnz * (2 * vb + 4) + 8 * N + 16 * d,
                  'wall_output_equals_resident_run': same})
        line += f"; host arrays -> resident matrix, sparse route: {t_sparse:.3f} s wall (of it canonical copy + tocsc on the host: {t_host:.3f} s)"
        del out
        # ---- dense route ----
        if 4 * N * d <= a.dense_max_gb * 1e9:
            # the cells as a dense host array: the densify kernel against mean 0, sd 1 writes exactly them
            dense_host = jsp.apply_csr(A, np.zeros(d), np.ones(d)).cpu().numpy().astype(np.float32 if a.dtype == 'f32' else np.float64)
            X = torch.from_numpy(dense_host).cuda()
            t_dk = timed(lambda: nv.standardise_columns(X), a.reps)
            del X
            torch.cuda.empty_cache()
            t_dense, dres = wall(lambda: nv.standardise_columns(torch.from_numpy(dense_host).cuda()))
            r['max_abs_difference_of_the_routes'] = float((dres[0] - got[0]).abs().max())
            del dres
            r.update({'dense_kernels_s': t_dk[0], 'dense_kernels_s_min_max': t_dk[1:], 'dense_wall_s': t_dense,
                      'dense_upload_bytes': dense_host.nbytes})
            line += (f"; dense route: jamie_col_stats + jamie_standardise {t_dk[0] * 1e3:.3f} ms ({t_dk[1] * 1e3:.3f}-{t_dk[2] * 1e3:.3f}), "
                     f"host array -> resident matrix {t_dense:.3f} s wall; max |sparse route - dense route| {r['max_abs_difference_of_the_routes']:.2e}")
            del dense_host
        else:
            line += f'; dense route skipped ({4 * N * d / 1e9:.1f} GB of dense fp32 above --dense-max-gb)'
        line += f"; standardise_csr output equals the resident run's: {same}"
        rows.append(r)
        print(line, flush=True)
        del got, A
        torch.cuda.empty_cache()
    print(json.dumps({'bench_sparse_input': rows, 'peak_bytes_per_s': peak, 'value_dtype': a.dtype}))


if __name__ == '__main__':
    main()
